"""The bits of the fp64 matrix-pipe Gram walk behind ``weight_correlation`` and ``stein``: sha256 digests of what the public
calls return on seeded inputs.  Needs the MI355X and the built library:

    python tests/golden/make_gram_bits.py --parent <commit>     ->  tests/golden/gram_bits.json

The file was recorded with the library of the commit BEFORE the Gram passes of csrc/corr_hip.inc and csrc/stein_hip.inc
came to share their pieces in csrc/gram_hip.inc; it carries that commit's hash and its library's source stamp.  The
library is built with -ffp-contract=off, so a later library that performs the same operations in the same order
reproduces every digest (``test_the_gram_walk_reproduces_the_recorded_bits`` in tests/test_weight_correlation.py and
tests/test_stein.py).

Shapes: the smallest at which the walk can go wrong.  TILE = 64 rows per block, CHUNK = 32 contracted elements per chunk.

  correlation  V in {17, 65, 130} (one partial tile; a full tile plus one row; three tile rows with off-diagonal block
               pairs) x n = 70 (two full chunks and a partial one) x {fp32, fp64} x {variable-major, observation-major,
               observation-major on every second sample of a longer stack} x a workspace that leaves {1, 3} splits;
               the batched path with R = 2 permuted replicates in one launch; one NaN and one Inf
  stein        S in {2, 33, 65} (4 rows; the X / G boundary at row 33 of 66; at row 65, inside the second tile of 130 rows)
               x D in {1, 33, 70} x {fp32, fp64} x {contiguous, row-strided column slices} x a workspace of {1, 3} slabs
               (as many splits where D has the chunks); one NaN in x and one Inf in the score
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(HERE))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PATH = os.path.join(HERE, "gram_bits.json")
N_OBS = 70
PICKS = 5
CORR_LAYOUTS = ("vmajor", "obs", "obs_strided")


def versions():
    return dict(torch=torch.__version__, rocm=str(torch.version.hip), numpy=np.__version__)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------- correlation

def corr_cases():
    "name -> (V, dtype, layout, slabs the workspace holds, special)"
    out = {}
    for V in (17, 65, 130):
        for dtype in ("float32", "float64"):
            for layout in CORR_LAYOUTS:
                for slabs in (1, 3):
                    out[f"v{V}_{dtype}_{layout}_sp{slabs}"] = (V, dtype, layout, slabs, "")
    out["v65_float32_vmajor_sp3_nan_inf"] = (65, "float32", "vmajor", 3, "bad")
    return out


def corr_stack(name):
    "the device stack of a case (variables on axis 0 of its shape, n = 70 observations), seeded by the case's position"
    V, dtype, layout, _, special = corr_cases()[name]
    rng = np.random.default_rng(sorted(corr_cases()).index(name) + 300)
    shape = (N_OBS, V) if layout == "vmajor" else (7, V, 10)
    fshape = (N_OBS, 1) if layout == "vmajor" else (7, 1, 10)
    w = (0.05 * (rng.standard_normal(shape) + 0.9 * rng.standard_normal(fshape))).astype(dtype)
    if special == "bad":                                     # placed as tests/test_weight_correlation.py's "bad" does
        w.reshape(-1)[7] = np.nan
        w.reshape(-1)[w.size - 3] = np.inf
    if layout == "obs_strided":
        base = rng.standard_normal((14, V, 10)).astype(dtype)
        base[::2] = w
        return torch.from_numpy(base).cuda()[::2]
    return torch.from_numpy(w).cuda()


def _offdiag_arrays(od, prefix=""):
    return {prefix + k: _sha(getattr(od, k)) for k in od._fields}


def corr_digests():
    "{case: {array: sha256}} of covariance + offdiag_stats, and of the batched permutation path"
    from bnn_priors_amd import weight_correlation as wc
    out = {}
    for name, (V, dtype, layout, slabs, _) in corr_cases().items():
        w = corr_stack(name)
        assert w.is_contiguous() == (layout != "obs_strided")
        g = wc._geometry(w, 0)
        assert (g.V, g.n, g.v_major) == (V, N_OBS, int(layout == "vmajor"))
        ws = slabs * 8 * V * V
        assert wc.splits(V, N_OBS, ws) == slabs
        c = wc.covariance(w, 0, workspace_bytes=ws)
        rec = {k: _sha(getattr(c, k)) for k in ("mean", "cov", "corr", "zero_variance", "nonfinite")}
        rec.update(_offdiag_arrays(wc.offdiag_stats(c.corr), "offdiag."))
        out[name] = rec
    # R = 2 replicates riding in one launch of the Gram kernel (3 splits: the default workspace holds them all)
    for V, dtype in ((17, "float64"), (65, "float32"), (130, "float32")):
        name = f"v{V}_{dtype}_obs_sp3"
        w = corr_stack(name)
        rng = np.random.default_rng(400 + V)
        tables = np.stack([np.stack([rng.permutation(N_OBS) for _ in range(V)]) for _ in range(2)]).astype(np.int64)
        tables = torch.from_numpy(tables).cuda()
        sp = wc.splits(V, N_OBS)
        assert sp == 3 and wc._batch_replicates(V, N_OBS, sp, w.element_size(), 2, wc.WORKSPACE_BYTES) == 2
        t = wc.independence_test(w, 0, perms=tables)
        rec = dict(null=_sha(t.null), p_rms=_sha(t.p_rms), p_max=_sha(t.p_max))
        rec.update(_offdiag_arrays(t.observed, "observed."))
        # ... and the two correlation matrices themselves, as independence_test forms them
        g = wc._geometry(w, 0)
        mean, bad = wc._mean(w, g)
        x = w.movedim(1, 0).reshape(V, N_OBS).contiguous()
        xp = torch.gather(x.unsqueeze(0).expand(2, V, N_OBS), 2, tables)
        _, corr2, zero2 = wc._gram(xp, wc._contiguous_geometry(V, N_OBS), 2, V * N_OBS, mean, bad, sp, 1, False)
        rec.update(corr=_sha(corr2), zero_variance=_sha(zero2))
        out[f"perm_r2_v{V}_{dtype}"] = rec
    return out


# ---------------------------------------------------------------------------------------------------------------- stein

def stein_cases():
    "name -> (S, D, dtype, layout, slabs the workspace holds, special)"
    out = {}
    for S in (2, 33, 65):
        for D in (1, 33, 70):
            for dtype in ("float32", "float64"):
                for layout in ("contig", "strided"):
                    for slabs in (1, 3):
                        if slabs == 1 or D > 32:             # (one chunk: the second workspace would repeat the first)
                            out[f"s{S}_d{D}_{dtype}_{layout}_sp{slabs}"] = (S, D, dtype, layout, slabs, "")
    out["s33_d70_float32_contig_sp3_nan_inf"] = (33, 70, "float32", "contig", 3, "bad")
    return out


def stein_inputs(name):
    "(x, score) of a case on the device: draws of N(0.3, 1) with the score of a nearby target"
    S, D, dtype, layout, _, special = stein_cases()[name]
    rng = np.random.default_rng(sorted(stein_cases()).index(name) + 500)
    z = rng.standard_normal((S, D))
    x, g = (z + 0.3).astype(dtype), (-(z * 1.1) + 0.2 * rng.standard_normal((S, D))).astype(dtype)
    if special == "bad":                                     # placed as tests/test_stein.py's "bad" does
        x[2, 1], g[5, 3] = np.nan, np.inf
    if layout == "strided":                                  # every second sample of a longer stack, a column slice
        bx, bg = (rng.standard_normal((2 * S, D + 9)).astype(dtype) for _ in range(2))
        bx[::2, 4:4 + D], bg[1::2, 2:2 + D] = x, g
        return torch.from_numpy(bx).cuda()[::2, 4:4 + D], torch.from_numpy(bg).cuda()[1::2, 2:2 + D]
    return torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()


def stein_digests():
    "{case: {array: sha256}} of kernel_matrix and the thinning order of 5 picks"
    from bnn_priors_amd import stein
    out = {}
    for name, (S, D, dtype, layout, slabs, _) in stein_cases().items():
        x, g = stein_inputs(name)
        assert x.is_contiguous() == (layout == "contig") and x.shape == g.shape == (S, D)
        ws = slabs * 8 * 4 * S * S
        assert stein.splits(S, D, ws) == min(slabs, -(-D // stein.CHUNK))
        k = stein.kernel_matrix(x, g, workspace_bytes=ws)
        out[name] = dict(K=_sha(k.K), r2=_sha(k.r2), nonfinite=_sha(k.nonfinite), thin=_sha(stein.thin(k, PICKS).indices))
    return out


def main():
    from bnn_priors_amd import _hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit whose library records the bits")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    rec = dict(versions=versions(), parent_commit=a.parent, library_sha=_hip.library_sha(), corr=corr_digests(),
               stein=stein_digests())
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out, "from library", rec["library_sha"], "of commit", a.parent, rec["versions"],
          len(rec["corr"]), "correlation and", len(rec["stein"]), "stein cases")


if __name__ == "__main__":
    main()
