"""CPU only: what tests/test_gpu_gan_ops_sweep.py relies on, checked without a GPU.

  Regime coverage    every table of tests/gan_ops_cases.py reaches every tag of its *_NEEDED set, and every entry's declared
                     tags equal the ones recomputed from the launch arithmetic.
  Exact inputs       from the tables' own inputs, sum |terms| < 2^24 for every exact case: any order of adding gives the fp64 sum.
  Replay shortcuts   the reshape / transpose index maps and the resize formula equal a naive loop.
  Bound headroom     a float32 numpy restatement of each kernel's own order (lane chains, the fold as written, slices, finish
                     groups) stays within HALF the stated bound on the tables' bounded inputs.  Two places cannot: lerp's three
                     roundings are nearly attained by some element (0.66, the count is tight), and a bf16 result attains the
                     half ulp of its one rounding -- there the f32 value before storing keeps the half, the stored one the bound.
  Bound sensitivity  the same restatement with one contribution removed (a lane, a pixel, a slice, a row, a channel quad, a
                     position) exceeds the bound on the bounded inputs and differs from the fp64 sum on the exact ones.
  The defect         the halving tree as it stood for every pl, applied to the non_pow2 bf16 cases, fails the exact comparison;
                     the fixed fold (the tree where pl is a power of two, serial otherwise) passes.
  Refusals           no refusal case of the GPU file could read or write out of range if its check were missing."""
import numpy as np
import pytest
import torch

from tests import gan_ops_cases as gc

U = gc.U
TABLES = [
    ("wgrad1x1_small f32", gc.WG32_CASES, gc.wg32_tags, gc.WG32_NEEDED),
    ("wgrad1x1_small bf16", gc.WGBF_CASES, gc.wgbf_tags, gc.WGBF_NEEDED),
    ("conv1x1 smallin", gc.SMALLIN_CASES, gc.smallin_tags, gc.SMALLIN_NEEDED),
    ("conv1x1 smallout", gc.SMALLOUT_CASES, gc.smallout_tags, gc.SMALLOUT_NEEDED),
    ("pixelnorm f32", gc.PN32_CASES, gc.pn_tags, gc.PN32_NEEDED),
    ("pixelnorm bf16", gc.PNBF_CASES, gc.pn_tags, gc.PNBF_NEEDED),
    ("mbstd f32", gc.MB32_CASES, gc.mb_tags, gc.MB_NEEDED),
    ("mbstd bf16", gc.MBBF_CASES, gc.mb_tags, gc.MB_NEEDED | {"both_halves"}),
    ("lerp / scale / act", gc.ALGEBRA_CASES, gc.algebra_tags, gc.ALGEBRA_NEEDED),
    ("dot_per_sample", gc.DOT_CASES, gc.dot_tags, gc.DOT_NEEDED),
    ("resize_nearest", gc.RESIZE_CASES, gc.resize_tags, gc.RESIZE_NEEDED),
    ("mosaic", gc.MOSAIC_CASES, gc.mosaic_tags, gc.MOSAIC_NEEDED),
    ("head_concat", gc.HEAD_CONCAT_CASES, gc.head_concat_tags, gc.HEAD_CONCAT_NEEDED),
    ("dense", gc.DENSE_CASES, gc.dense_tags, gc.DENSE_NEEDED),
    ("dense_wgrad", gc.DENSE_WGRAD_CASES, gc.dense_wgrad_tags, gc.DENSE_WGRAD_NEEDED),
]


def _ids(cases):
    return ["-".join(str(v) for v in c) for c, _ in cases]


def frac(got, ref, bound):
    """the worst |got - ref| as a fraction of the bound (a zero bound with a zero error counts as 0)"""
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())


# ---- regime coverage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cases,tags_of,needed", TABLES, ids=[t[0] for t in TABLES])
def test_tables_reach_every_regime(name, cases, tags_of, needed):
    reached = set()
    for c, declared in cases:
        assert tags_of(c) == declared, "%s %r: declared %s, the launch arithmetic gives %s" % (
            name, c, sorted(declared), sorted(tags_of(c)))
        reached |= declared
    assert not needed - reached, "%s: no case reaches %s" % (name, sorted(needed - reached))


def test_launch_constants_are_those_of_the_sources():
    """the caps differ between the files: each named constant is read back from the .hip source it restates"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sequitr_amd", "csrc")
    f32, bf = (open(os.path.join(csrc, n)).read() for n in ("sq_gan_ops.hip", "sq_gan_bf16.hip"))
    for src, grid, small in ((f32, gc.GRID_CAP_F32, gc.SMALL_CAP_F32), (bf, gc.GRID_CAP_BF16, gc.SMALL_CAP_BF16)):
        assert int(re.search(r"grid_for\(int64_t items\) \{.*?if \(b > (\d+)\)", src, re.S).group(1)) == grid
        assert int(re.search(r"small_blocks\(int64_t npix\) \{.*?b > (\d+) \?", src, re.S).group(1)) == small
    assert int(re.search(r"DOT_SLICES = (\d+)", f32).group(1)) == gc.DOT_SLICES
    assert (int(re.search(r"MB_B = (\d+)", f32).group(1)), int(re.search(r"MB_BT = (\d+)", f32).group(1)),
            int(re.search(r"MB_T = (\d+)", f32).group(1))) == (gc.MB_B, gc.MB_BT, gc.MB_T)
    dense = open(os.path.join(csrc, "sq_dense.hip")).read()
    assert tuple(int(re.search(r"constexpr int %s = (\d+)" % n, dense).group(1)) for n in ("DK", "DM", "WK")) == (gc.DK, gc.DM, gc.WK)


def test_tree_fold_table():
    """the halving tree reaches every lane exactly where pl is a power of two; the issue's table otherwise"""
    table = {24: (85, 64), 40: (51, 32), 48: (42, 32), 56: (36, 32), 72: (28, 16), 96: (21, 16), 120: (17, 16), 192: (10, 8),
             320: (6, 4)}
    for C, (pl, reached) in table.items():
        assert 256 // (C // 8) == pl and gc.tree_lanes_reached(pl) == reached
    for pl in range(1, 257):
        assert (gc.tree_lanes_reached(pl) == pl) == gc._pow2(pl)


# ---- exact inputs --------------------------------------------------------------------------------------------------------
def test_exact_inputs_stay_below_2_24():
    worst = 0.0
    for (npix, Ca, Cb), _ in gc.WG32_CASES:
        a, b = gc.wg_inputs(npix, Ca, Cb, True, False)
        worst = max(worst, float(gc.wg_ref64(a, b)[1].max()))
    for (npix, Ca, C, a_none, asum, scale), _ in gc.WGBF_CASES:
        a, b = gc.wg_inputs(npix, Ca, C, True, True, a_none)
        assert torch.equal(b.to(gc.BF16).to(gc.F32), b), "b must be exact in bf16"
        _, terms, _, asum_terms = gc.wg_ref64(a, b, 1.0)       # before the (power-of-two) scale
        worst = max(worst, float(terms.max()), float(asum_terms.max()))
        assert scale in (1.0, 0.5)
    for c, _ in gc.DOT_CASES:
        a, b = gc.dot_inputs(c, True)
        worst = max(worst, float((a.double() * b.double()).abs().sum(1).max()))
    for c, _ in gc.DENSE_CASES:
        i = gc.dense_inputs(c, True)
        assert c[5] in (1.0, 0.5)
        worst = max(worst, float(gc.dense_ref64(i, None, 1.0)[1].max()))
    for c, _ in gc.DENSE_WGRAD_CASES:
        i = gc.dense_wgrad_inputs(c, True)
        assert c[4] in (1.0, 0.5)
        dw, dwt, db, dbt = gc.dense_wgrad_ref64(i, 3, 1.0)
        worst = max(worst, float(dwt.max()), float(dbt.max()))
    for c in gc.MB_EXACT_CASES:
        groups, n, P, cells = c
        i = gc.mb_exact_inputs(c)
        assert gc._pow2(n) and gc._pow2(P) and n % 2 == 0
        s, d = gc.mb_stat64(i["x"], groups)
        assert bool((s == 1.0).all()) and torch.equal(d.reshape(-1, P), i["x"].double())
        worst = max(worst, float(i["dy"].abs().reshape(groups, -1).sum(1).max()))
    print("largest sum |terms| of an exact case: %.3g of 2^24 = %.3g" % (worst, 2.0 ** 24))
    assert worst < 2.0 ** 24


# ---- replay shortcuts ----------------------------------------------------------------------------------------------------
def test_replay_shortcuts_equal_naive_loops():
    for c, _ in gc.RESIZE_CASES:
        x = gc.resize_input(c)
        assert torch.equal(gc.resize_replay(x, c[3], c[4]), gc.resize_loop(x, c[3], c[4])), c
    # half coordinates round away from zero: 4 -> 3 has the source coordinate 1.5 at output 1, which reads row 2
    assert gc._resize_src(4, 3)[0].tolist() == [0, 2, 3] and gc._resize_src(8, 4)[0].tolist() == [0, 2, 5, 7]
    for c, _ in gc.MOSAIC_CASES:
        x = gc.mosaic_input(c)
        m = gc.mosaic_replay(x, c[4], c[5])
        assert torch.equal(m, gc.mosaic_loop(x, c[4], c[5])), c
        assert int(gc.mosaic_seam_mask(c).sum()) == m.numel() - x.numel()
    N, P, C = 2, 3, 8
    i = gc.head_concat_inputs((N, P, C))
    flat = gc.head_concat_replay(i["conv"], i["mb"])
    for n in range(N):
        for p in range(P):
            row = flat[n, p * (C + 1):(p + 1) * (C + 1)]
            assert torch.equal(row[:C], i["conv"][n, p].float()) and float(row[C]) == float(i["mb"][n, p])
    dconv, dmb = gc.head_split_replay(flat, N, P, C)
    assert torch.equal(dconv, i["conv"]) and torch.equal(dmb, i["mb"])


def test_fp64_definitions_agree_with_autograd():
    """the closed forms of pn_ref64 and wgan_bwd_ref64 against automatic differentiation of the definitions"""
    i = gc.pn_inputs((False, 12, 5))
    x = i["x"].double().requires_grad_(True)
    g = i["g"].double().requires_grad_(True)
    eps = float(np.float32(gc.PN_EPS))
    y = x / torch.sqrt((x * x).mean(1, keepdim=True) + eps)
    (dx,) = torch.autograd.grad((y * g).sum(), x, create_graph=True)
    dg, dx2 = torch.autograd.grad((dx * i["v"].double()).sum(), (g, x))
    r = gc.pn_ref64(i, False)
    for name, want in (("fwd", y), ("bwd", dx), ("dg", dg), ("dx2", dx2)):
        assert torch.allclose(r[name][0], want.detach(), rtol=1e-10, atol=1e-12), name
    w = gc.wgan_inputs(32)
    w["gn2"][1] = 0.3                                           # away from the root's singular point for autograd
    Dz, Dx, gn2 = (w[k].double().requires_grad_(True) for k in ("Dz", "Dx", "gn2"))
    ex = (gn2.sqrt() - 1.0).clamp(min=0.0)
    d = (-Dx + Dz + float(np.float32(10.0)) * ex * ex + float(np.float32(0.001)) * Dx * Dx).mean()
    gl = (-Dz).mean()
    gd, gg = 0.7, -1.3
    grads = torch.autograd.grad(float(np.float32(gd)) * d + float(np.float32(gg)) * gl, (Dz, Dx, gn2))
    rb = gc.wgan_bwd_ref64(w, gd, gg)
    for name, want in zip(("dDz", "dDx", "dgn2"), grads):
        assert torch.allclose(rb[name][0], want, rtol=1e-10, atol=1e-14), name
    dref, _, gref, _ = gc.wgan_ref64(w)
    assert abs(float(dref) - float(d.detach())) < 1e-12 and abs(float(gref) - float(gl.detach())) < 1e-12


# ---- image-side small weight gradients: headroom, sensitivity, the defect -----------------------------------------------------
def _wg_check(a, b, L, unit, cap, scale, exact, fold="fixed", drop=None):
    """(fraction of the bound for m, for asum; equal to fp64 on m, on asum)"""
    m64, terms, s64, sterms = gc.wg_ref64(a, b, scale)
    m, asum = gc.wg_restated(a, b, unit, cap, fold, scale, drop)
    return (frac(m, m64, L.k(scale) * U * terms), frac(asum, s64, L.k_asum() * U * sterms),
            bool((m.double() == m64).all()), bool((asum.double() == s64).all()))


@pytest.mark.parametrize("c", [c for c, _ in gc.WG32_CASES], ids=_ids(gc.WG32_CASES))
def test_wgrad_small_f32_bound_and_sensitivity(c):
    npix, Ca, Cb = c
    L = gc.wg32_launch(c)
    a, b = gc.wg_inputs(npix, Ca, Cb, False, False)
    fm, _, _, _ = _wg_check(a, b, L, 4, gc.SMALL_CAP_F32, 1.0, False)
    assert fm <= 0.5, "the restated kernel uses %.3f of the bound k = %d" % (fm, L.k())
    lane = min(L.step, npix) // 2
    assert _wg_check(a, b, L, 4, gc.SMALL_CAP_F32, 1.0, False, drop=("lane", lane))[0] > 1.0
    a, b = gc.wg_inputs(npix, Ca, Cb, True, False)
    assert _wg_check(a, b, L, 4, gc.SMALL_CAP_F32, 1.0, True)[2]
    p = int((a[:, 0] * b[:, 0]).nonzero()[-1])
    assert not _wg_check(a, b, L, 4, gc.SMALL_CAP_F32, 1.0, True, drop=("pixel", p))[2]


@pytest.mark.parametrize("c", [c for c, _ in gc.WGBF_CASES], ids=_ids(gc.WGBF_CASES))
def test_wgrad_small_bf16_bound_sensitivity_and_the_defect(c):
    npix, Ca, C, a_none, want_asum, scale = c
    L = gc.wgbf_launch(c)
    cap = gc.SMALL_CAP_BF16
    a, b = gc.wg_inputs(npix, Ca, C, False, True, a_none)
    fm, fs, _, _ = _wg_check(a, b, L, 8, cap, scale, False)
    assert fm <= 0.5 and fs <= 0.5, "the restated kernel uses %.3f (m, k = %d) and %.3f (asum, k = %d) of the bounds" % (
        fm, L.k(scale), fs, L.k_asum())
    lane = min(L.step, npix) // 2
    assert _wg_check(a, b, L, 8, cap, scale, False, drop=("lane", lane))[0] > 1.0
    # (asum's serial fold makes its k as large as pl: one lane of it can stay inside the bound; the exact inputs below see it)
    a, b = gc.wg_inputs(npix, Ca, C, True, True, a_none)
    _, _, em, es = _wg_check(a, b, L, 8, cap, scale, True)
    assert em and es, "the fixed fold must equal fp64 on the exact inputs"
    p = int(((b[:, 0] if a is None else a[:, 0] * b[:, 0]) != 0).nonzero()[-1])
    dropped = _wg_check(a, b, L, 8, cap, scale, True, drop=("pixel", p))
    assert not dropped[2] and (a_none or not dropped[3])
    # the halving tree for every pl (the kernel before the fix): complete exactly where pl is a power of two
    _, _, tree_m, tree_s = _wg_check(a, b, L, 8, cap, scale, True, fold="tree")
    assert tree_s, "asum is folded serially either way"
    assert tree_m == L.tree, "C / 8 = %d, pl = %d: the tree reaches %d lanes" % (L.groups, L.pl, gc.tree_lanes_reached(L.pl))
    if "non_pow2" in gc.wgbf_tags(c):
        assert not tree_m
        a, b = gc.wg_inputs(npix, Ca, C, False, True, a_none)
        assert _wg_check(a, b, L, 8, cap, scale, False, fold="tree")[0] > 1.0, "the bounded comparison catches it too"


def test_image_conv_bounds_hold_for_a_naive_f32_evaluation():
    """smallin / smallout: the fmaf chain in channel order from 0, in numpy float32, within half the bound"""
    f = np.float32
    for cases, out in ((gc.SMALLIN_CASES, False), (gc.SMALLOUT_CASES, True)):
        for c, _ in cases:
            npix, Cs, C, bias, act = c
            if npix > 2000:
                continue
            i = gc.image_conv_inputs(c, out)
            x, w = i["x"].numpy(), i["w"].numpy() * f(gc.IMAGE_WSCALE)
            acc = np.zeros((npix, w.shape[1]), f)
            for k in range(x.shape[1]):
                acc = gc._fma32(w[k][None, :], x[:, k:k + 1], acc)
            if bias:
                acc = acc + i["bias"].numpy()
            if gc.SLOPE[act] != 1.0:
                acc = np.where(acc > 0, acc, acc * f(gc.SLOPE[act]))
            ref, terms = gc.image_conv_ref64(i, act)
            k = gc.smallout_k(C) if out else gc.smallin_k(Cs)
            assert frac(torch.from_numpy(acc), ref, k * U * terms) <= 0.5, c
            acc[:, 0] = acc[:, 0] - (w[0, 0] * x[:, 0])         # one term removed
            assert frac(torch.from_numpy(acc), ref, k * U * terms) > 1.0, c


# ---- pixel norm ----------------------------------------------------------------------------------------------------------
_PN_SMALL = [t for t in gc.PN32_CASES + gc.PNBF_CASES if t[0][2] < 1000]


@pytest.mark.parametrize("c", [c for c, _ in _PN_SMALL], ids=_ids(_PN_SMALL))
def test_pixelnorm_bound_and_sensitivity(c):
    bf, C, npix = c
    i = gc.pn_inputs(c)
    r = gc.pn_ref64(i, bf)

    def fractions(drop=None):
        out = {}
        for act in gc.ACTS:
            got = gc.pn_restated(i, bf, act, drop_piece=drop)
            e, b = gc.pn_gate(r["bwd"][0], r["bwd"][1], i["x"], act, bf)
            out["bwd/%s" % act] = frac(got["bwd"], e, b)
        for name in ("fwd", "dg", "dx2"):
            e, b = r[name]
            out[name] = frac(got[name], e, gc.pn_store_bound(e, b) if bf else b)
        return out

    used = fractions()
    # a bf16 result is one rounding of a value that is within the f32 bound: the half ulp it adds is attained, so only the f32
    # part of the bound can keep a factor of two
    limit = 1.0 if bf else 0.5
    assert max(used.values()) <= limit, "the restated kernels use %r of the bounds" % (used,)
    if bf:                                                      # the f32 values before they are stored keep the factor of two
        got = gc.pn_restated(i, True, None, store=False)
        raw = {name: frac(got[name], *r[name]) for name in ("fwd", "bwd", "dg", "dx2")}
        assert max(raw.values()) <= 0.5, "before storing, the restated kernel uses %r of the f32 bounds" % (raw,)
    pieces = C // (8 if bf else 4)
    if pieces > 1:                                              # with one piece there is nothing left to sum
        dropped = fractions(drop=pieces - 1)
        assert min(dropped.values()) > 1.0, "one channel piece removed stays inside %r" % (dropped,)


def test_pixelnorm_inputs_exercise_the_gate():
    for cases in (gc.PN32_CASES, gc.PNBF_CASES):
        for c, _ in cases:
            x = gc.pn_inputs(c)["x"]
            assert bool((x > 0).any()) and bool((x < 0).any()) and bool((x == 0).any()), c


# ---- minibatch stdev -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c, _ in gc.MB32_CASES + gc.MBBF_CASES], ids=_ids(gc.MB32_CASES + gc.MBBF_CASES))
def test_mbstd_bound_and_sensitivity(c):
    bf, groups, n, P, cells = c
    i = gc.mb_inputs(c)
    ref, bnd = gc.mb_ref64(i, groups), gc.mb_bounds(i, groups)
    got = gc.mb_restated(i, groups)                             # the f32 values: half of the f32 bounds
    used = {name: frac(got[name], ref[name], bnd[name]) for name in ("y", "dx", "ddy", "dx2")}
    assert max(used.values()) <= 0.5, "the restated kernels use %r of the bounds" % (used,)
    if bf:                                                      # as stored: the half ulp of the rounding is attained
        got = gc.mb_restated(i, groups, bf=True)
        for name in ("dx", "dx2"):
            assert frac(got[name], ref[name], bnd[name] + gc.HALF_BF16_ULP * (ref[name].abs() + bnd[name])) <= 1.0, name
    got = gc.mb_restated(i, groups, drop_position=P // 2)
    assert frac(got["y"], ref["y"], bnd["y"]) > 1.0 and frac(got["ddy"], ref["ddy"], bnd["ddy"]) > 1.0
    got = gc.mb_restated(i, groups, drop_dy=n * cells - 1)
    assert frac(got["dx"], ref["dx"], bnd["dx"]) > 1.0 and frac(got["dx2"], ref["dx2"], bnd["dx2"]) > 1.0


@pytest.mark.parametrize("c", gc.MB_EXACT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_mbstd_exact_dy_sum(c):
    groups, n, P, cells = c
    i = gc.mb_exact_inputs(c)
    want = (i["dy"].double().reshape(groups, -1).sum(1) / (P * n)).reshape(groups, 1, 1) * i["x"].double().reshape(groups, n, P)
    assert torch.equal(gc.mb_restated(i, groups)["dx"].double(), want.reshape(-1, P))
    assert torch.allclose(gc.mb_ref64({"x": i["x"], "dy": i["dy"], "v": i["x"]}, groups)["dx"], want.reshape(-1, P), rtol=1e-12, atol=0)
    nz = int(i["dy"].reshape(groups, -1)[0].nonzero()[-1])
    assert not torch.equal(gc.mb_restated(i, groups, drop_dy=nz)["dx"].double(), want.reshape(-1, P))


# ---- dot_per_sample and dense ---------------------------------------------------------------------------------------------
def _columns(i, K, keep=48):
    """output columns are independent in both dense kernels: the restatement of the workload-sized cases (K = 8208) walks the
    first `keep` of them, over the whole reduction"""
    if K < 1000:
        return i
    return {k: (t if (t is None or k == "x") else (t[..., :keep].contiguous())) for k, t in i.items()}


@pytest.mark.parametrize("c", [c for c, _ in gc.DOT_CASES], ids=_ids(gc.DOT_CASES))
def test_dot_per_sample_bound_and_sensitivity(c):
    a, b = gc.dot_inputs(c, False)
    ref, terms = (a.double() * b.double()).sum(1), (a.double() * b.double()).abs().sum(1)
    bound = gc.dot_k(c[1]) * U * terms
    assert frac(gc.dot_restated(a, b), ref, bound) <= 0.5
    assert frac(gc.dot_restated(a, b, drop_slice=gc.DOT_SLICES - 1), ref, bound) > 1.0
    a, b = gc.dot_inputs(c, True)
    ref = (a.double() * b.double()).sum(1)
    assert torch.equal(gc.dot_restated(a, b).double(), ref)
    a[:, -1], b[:, -1] = 1.0, 1.0                               # the last slice now holds a nonzero term for certain
    assert not torch.equal(gc.dot_restated(a, b, drop_slice=gc.DOT_SLICES - 1).double(), (a.double() * b.double()).sum(1))


@pytest.mark.parametrize("c", [c for c, _ in gc.DENSE_CASES], ids=_ids(gc.DENSE_CASES))
def test_dense_bound_and_sensitivity(c):
    M, K, N, bias, act, wscale = c
    i = _columns(gc.dense_inputs(c, False), K)
    ref, terms = gc.dense_ref64(i, act, gc.DENSE_BOUNDED_WSCALE)
    bound = gc.dense_k(K) * U * terms
    assert frac(gc.dense_restated(i, act, gc.DENSE_BOUNDED_WSCALE), ref, bound) <= 0.5
    assert frac(gc.dense_restated(i, act, gc.DENSE_BOUNDED_WSCALE, drop_slice=0), ref, bound) > 1.0
    if act != "leaky":                                          # 0.2 v is not exact
        i = _columns(gc.dense_inputs(c, True), K)
        ref, _ = gc.dense_ref64(i, act, wscale)
        assert torch.equal(gc.dense_restated(i, act, wscale).double(), ref)
        assert not torch.equal(gc.dense_restated(i, None, wscale, drop_slice=0).double(), gc.dense_ref64(i, None, wscale)[0])


@pytest.mark.parametrize("c", [c for c, _ in gc.DENSE_WGRAD_CASES], ids=_ids(gc.DENSE_WGRAD_CASES))
def test_dense_wgrad_bound_and_sensitivity(c):
    M, K, N, accumulate, scale, want_db = c
    i = _columns(gc.dense_wgrad_inputs(c, False), K)
    dw64, dwt, db64, dbt = gc.dense_wgrad_ref64(i, accumulate, scale)
    k = gc.dense_wgrad_k(M)
    dw, db = gc.dense_wgrad_restated(i, accumulate, scale)
    assert frac(dw, dw64, k * U * dwt) <= 0.5 and frac(db, db64, k * U * dbt) <= 0.5
    dw, db = gc.dense_wgrad_restated(i, accumulate, scale, drop_row=M - 1)
    assert frac(dw, dw64, k * U * dwt) > 1.0 and frac(db, db64, k * U * dbt) > 1.0
    i = _columns(gc.dense_wgrad_inputs(c, True), K)
    dw64, _, db64, _ = gc.dense_wgrad_ref64(i, accumulate, scale)
    dw, db = gc.dense_wgrad_restated(i, accumulate, scale)
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
    i["x"][0, 0], i["dy"][0, 0] = 1.0, 1.0
    dw64, _, db64, _ = gc.dense_wgrad_ref64(i, accumulate, scale)
    dw, db = gc.dense_wgrad_restated(i, accumulate, scale, drop_row=0)
    assert not torch.equal(dw.double(), dw64) and not torch.equal(db.double(), db64)


# ---- lerp / losses: the bounds against a plain float32 evaluation -------------------------------------------------------------
def test_lerp_and_wgan_bounds_hold_in_float32():
    f = np.float32
    i = gc.algebra_inputs(gc.ALGEBRA_CASES[1][0])
    a, b = i["a"].numpy(), i["b"].numpy()
    for al in (f(gc.LERP_ALPHA), i["per"].numpy()[:, None]):
        y = al * a + (f(1.0) - al) * b
        ref, bound = gc.lerp_ref64(i["a"], i["b"], gc.LERP_ALPHA if np.ndim(al) == 0 else i["per"])
        # three roundings, each nearly attained by some element of 4000: the count is tight, and half of it is not to be had
        # without inflating it (0.66 here); the sums below keep their factor of two
        assert frac(torch.from_numpy(y.astype(f)), ref, bound) <= 1.0
        assert frac(torch.from_numpy((al * a).astype(f)), ref, bound) > 1.0
    for N in gc.WGAN_N:
        w = gc.wgan_inputs(N)
        if N > 2:
            assert float(w["gn2"][0]) == 1.0 and float(w["gn2"][1]) == 0.0
        Dz, Dx, gn2 = (w[k].numpy() for k in ("Dz", "Dx", "gn2"))
        ex = np.maximum(np.sqrt(gn2) - f(1.0), f(0.0))
        d = ((-Dx + Dz) + f(10.0) * (ex * ex)) + f(0.001) * (Dx * Dx)
        th_d, th_g = np.zeros(gc.MB_T, f), np.zeros(gc.MB_T, f)
        for base in range(0, N, gc.MB_T):
            n = min(gc.MB_T, N - base)
            th_d[:n] = th_d[:n] + d[base:base + n]
            th_g[:n] = th_g[:n] + -Dz[base:base + n]
        got_d, got_g = gc._block_tree(th_d) / f(N), gc._block_tree(th_g) / f(N)
        dref, db, gref, gb = gc.wgan_ref64(w)
        assert abs(float(got_d) - float(dref)) <= 0.5 * float(db) and abs(float(got_g) - float(gref)) <= 0.5 * float(gb), N
        th_d[0] = 0.0                                           # one thread's share removed
        assert abs(float(gc._block_tree(th_d) / f(N)) - float(dref)) > float(db) or float(d[0]) == 0.0, N


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_no_refusal_could_go_out_of_range():
    """every refused call's wrong operand holds at least what a launch sized by the others would have covered"""
    names = set()
    for name, operand, has, covered in gc.REFUSALS:
        assert has >= covered, "%s: %s has %d elements, a launch would cover %d" % (name, operand, has, covered)
        names.add(name)
    assert len(names) == len(gc.REFUSALS)
