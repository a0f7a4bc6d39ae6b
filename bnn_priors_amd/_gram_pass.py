"""What ``weight_correlation`` and ``stein`` share on the host side of their fp64 Gram passes (``csrc/gram_hip.inc``)."""


def splits(V, length, workspace_bytes, tile, chunk, max_splits, target_blocks):
    """Workgroups that share the chunks of one block pair of a V x V Gram matrix contracted over ``length`` elements
    (``gram::splits``); 0 if the workspace holds no V x V doubles."""
    nb = -(-V // tile)
    return max(0, min(-(-length // chunk), max_splits, target_blocks // (nb * (nb + 1) // 2),
                      workspace_bytes // (8 * V * V)))


def check_workspace_bytes(workspace_bytes):
    if isinstance(workspace_bytes, bool) or not isinstance(workspace_bytes, int) or workspace_bytes < 0:
        raise ValueError(f"workspace_bytes = {workspace_bytes!r} must be a non-negative integer")
