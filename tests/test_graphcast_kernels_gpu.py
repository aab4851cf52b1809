"""The GraphCast building blocks of include/skyrim_graphcast.h (csrc/graphcast_ops.hip) at the edges the engine never reaches, each
against its float64 restatement in tests/_graphcast_reference.py and called the way the engine calls them, torch.ops.skyrim_hip.gc_*
(ctypes on the library where the op cannot express a case): skgc_gather_gemm at the edges of its 128 x 256 x 32 tile, with one to three
sources, K tails, leading dimensions above the width, misaligned rows, the per-k affine and swish far out; skgc_layer_norm up to N = 1024
with every aliasing the header allows, offset and constant rows; skgc_segment_sum with empty runs, a run of 1000 and rows nobody owns;
skgc_prepare_weight_perm8 + skgc_linear_layer_norm over K and row tails, offset pre-norm rows and W = I; skgc_sum_linear_layer_norm in
every group mode and against the two kernels it replaces; the documented argument refusals.  Every output starts as NaN with a margin
past its end: rows the call does not own and the margin are still NaN afterwards, and a refused call leaves all of it NaN.  Weights span
1e-3 .. 10 and hold no fp16 number, so a dropped lo plane shows (tests/test_graphcast_cpu.py shows that the bounds used here catch it)."""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import _graphcast_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 64                    # NaN elements past the end of every output
SPARE = 2                      # NaN rows past the rows a call owns
U = 2.0 ** -24                 # fp32 unit roundoff
L = 512
E_ARG = "invalid argument"


def _hip():
    from skyrim_amd import ops
    return ops.hip


def _lib():
    from skyrim_amd.graphcast import engine
    return engine.load_library()


def _stream():
    from skyrim_amd import native
    return native.stream(torch.device(DEV))


def _nan(n, dtype=torch.float32):
    return torch.full((n + MARGIN,), float("nan"), device=DEV, dtype=dtype)


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _take(out, rows, N):
    """The rows a call owns, on the host; everything behind them must still be NaN."""
    torch.cuda.synchronize()
    o = out.cpu()
    assert _all_nan(o[rows * N:]), "a write past the rows of the call"
    return o[:rows * N].view(rows, N)


def _refused(call, out):
    with pytest.raises(RuntimeError, match=E_ARG):
        call()
    torch.cuda.synchronize()
    assert _all_nan(out), "a refused call wrote to its output"


@pytest.fixture(scope="module")
def prep():
    """Prepared weights, one per shape and layout for the whole module: hilo(N, K) = sksfno_prepare_weight's planes of
    R.weight_for(N, K) (what skgc_gather_gemm reads), perm8(K) = skgc_prepare_weight_perm8's of R.weight_for(512, K)."""
    from skyrim_amd import native
    from skyrim_amd.sfno import engine as sf
    cache = {}

    class Prep:
        @staticmethod
        def hilo(N, K, w=None, key=None):
            k = ("hilo", N, K, key)
            if k not in cache:
                cache[k] = native.HiLoWeight(torch.device(DEV), sf.load_library().sksfno_prepare_weight, R.weight_for(N, K) if w is None else w)
            return cache[k]

        @staticmethod
        def perm8(K, w=None, key=None):
            """(planes, plane, ldw); ldw = K + 8 for K = 24 and 520, so that padding columns exist."""
            k = ("perm8", K, key)
            if k not in cache:
                ldw = K + 8 if K in (24, 520) else K
                planes = torch.full((2 * L * ldw,), float("nan"), dtype=torch.float16, device=DEV)
                wd = _d(R.weight_for(L, K) if w is None else w)
                rc = _lib().skgc_prepare_weight_perm8(wd.data_ptr(), L, K, planes.data_ptr(), L * ldw, ldw, _stream())
                torch.cuda.synchronize()
                assert rc == 0 and not torch.isnan(planes).any()
                cache[k] = (planes, L * ldw, ldw)
            return cache[k]

    return Prep


# ---- skgc_gather_gemm ---------------------------------------------------------------------------------------------------------------- #
def run_gather(c, W, act):
    M, N = c["M"], c["N"]
    out = _nan((M + SPARE) * N)
    _hip().gc_gather_gemm([_d(s) for s in c["srcs"]], [_d(i) for i in c["idxs"]], c["widths"], W.buf, W.plane, W.ldw, _d(c["bias"]), out, M, N, act,
                          _d(c["kscale"]), _d(c["kshift"]))
    return _take(out, M, N)


@pytest.mark.parametrize("N", [72, 256, 264])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_gather_gemm_tile_edges(prep, M, N):
    c = R.shape_case(M, N)
    for act in (0, 2):
        err = R.assert_close(run_gather(c, prep.hilo(N, c["K"]), act), R.gather_ref(c, act), R.BAR3, f"gather_gemm M={M} N={N} act={act}")
        print(f"ERR gather_gemm M={M} N={N} act={act} {err:.3e} / {R.BAR3:.1e}")


def test_gather_gemm_odd_n_is_right_or_refused(prep):
    """The header puts no condition on N: N = 257 (one column into the second 256-wide tile, rows that are not 16-byte aligned) is
    computed correctly, or refused with SKGC_E_ARG -- never a silent wrong answer."""
    c = R.gather_case((16, 8, 8), 129, 257, seed=1257, idx_kinds=(None, "rand", "rand"))
    W = prep.hilo(257, 32)
    try:
        got = run_gather(c, W, 2)
    except RuntimeError as e:
        assert E_ARG in str(e)
        return
    err = R.assert_close(got, R.gather_ref(c, 2), R.BAR3, "gather_gemm N=257")
    print(f"ERR gather_gemm N=257 {err:.3e} / {R.BAR3:.1e}")


WIDTHS = [(21,), (40,), (32, 8), (16, 8), (8, 8, 5), (16, 8, 8)]
KINDS = {"none": (None, None, None), "some": (None, "rand", None), "all": ("rand", "rand", "rand"), "repeat": ("repeat", "rand", "repeat"),
         "last": ("last", "last", "last")}


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_gather_gemm_sources_widths_and_index_arrays(prep, widths, kinds):
    """One, two and three sources; an index array on none, some and all of them, one that repeats a row for every m, one that names the
    source's last row for every m; a last width that is not a multiple of 8."""
    if kinds == "some" and len(widths) == 1:
        kinds = "all"
    c = R.gather_case(widths, 129, 72, seed=1500 + 10 * sum(widths) + len(widths), idx_kinds=KINDS[kinds][:len(widths)])
    err = R.assert_close(run_gather(c, prep.hilo(72, c["K"]), 2), R.gather_ref(c, 2), R.BAR3, f"gather_gemm widths={widths} idx={kinds}")
    print(f"ERR gather_gemm widths={widths} idx={kinds} {err:.3e} / {R.BAR3:.1e}")


def test_gather_gemm_production_shape(prep):
    c = R.gather_case((512, 512, 512), 130, 512, seed=1536, n_rows=(None, 40, 9), idx_kinds=(None, "rand", "rand"))
    err = R.assert_close(run_gather(c, prep.hilo(512, 1536), 2), R.gather_ref(c, 2), R.BAR3, "gather_gemm 130 x 512 x 1536")
    print(f"ERR gather_gemm production {err:.3e} / {R.BAR3:.1e}")


def test_gather_gemm_leading_dimensions_and_misaligned_rows(prep):
    """ld > width; and leading dimensions of 43 and 11 floats, where three rows in four are not 16-byte aligned and the loader reads
    element by element: the same values through aligned rows give the same bits."""
    c = R.gather_case((16, 8, 8), 129, 72, seed=1601, idx_kinds=(None, "rand", "rand"), lds=(24, 8, 20))
    err = R.assert_close(run_gather(c, prep.hilo(72, 32), 0), R.gather_ref(c, 0), R.BAR3, "gather_gemm ld > width")
    print(f"ERR gather_gemm ld>width {err:.3e} / {R.BAR3:.1e}")
    odd = R.gather_case((32, 8), 129, 72, seed=1602, idx_kinds=("rand", None), lds=(43, 11))
    even = dict(odd, srcs=[F.pad(odd["srcs"][0], (0, 5)), F.pad(odd["srcs"][1], (0, 1))])            # ld 48 and 12: every row aligned
    a, b = run_gather(odd, prep.hilo(72, 40), 2), run_gather(even, prep.hilo(72, 40), 2)
    err = R.assert_close(a, R.gather_ref(odd, 2), R.BAR3, "gather_gemm odd ld")
    print(f"ERR gather_gemm odd-ld {err:.3e} / {R.BAR3:.1e}")
    assert torch.equal(a, b), "the element-wise branch of the loader differs from the 16-byte branch on the same values"


@pytest.mark.parametrize("widths", R.AFFINE_WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_gather_gemm_per_k_affine_with_a_k_tail(prep, widths):
    """Shifts of order 10 on K = 21 and K = 40, with act 0 and 2; act 1 (GELU: not this kernel's) is refused."""
    c = R.affine_case(widths)
    W = prep.hilo(72, c["K"])
    for act in (0, 2):
        err = R.assert_close(run_gather(c, W, act), R.gather_ref(c, act), R.BAR3, f"gather_gemm affine K={c['K']} act={act}")
        print(f"ERR gather_gemm affine K={c['K']} act={act} {err:.3e} / {R.BAR3:.1e}")
    out = _nan(129 * 72)
    args = ([_d(s) for s in c["srcs"]], [_d(i) for i in c["idxs"]], c["widths"], W.buf, W.plane, W.ldw, _d(c["bias"]), out, 129, 72)
    _refused(lambda: _hip().gc_gather_gemm(*args, 1, _d(c["kscale"]), _d(c["kshift"])), out)
    _refused(lambda: _hip().gc_gather_gemm(*args, 2, _d(c["kscale"]), None), out)                   # a scale without its shift


def test_gather_gemm_refuses_an_inner_width_that_is_no_multiple_of_8(prep):
    c = R.gather_case((5, 8), 5, 72, seed=1700, idx_kinds=(None, None))
    W = prep.hilo(72, 21)
    out = _nan(5 * 72)
    _refused(lambda: _hip().gc_gather_gemm([_d(s) for s in c["srcs"]], [None, None], [5, 8], W.buf, W.plane, W.ldw, _d(c["bias"]), out, 5, 72, 2, None, None), out)


def test_gather_gemm_swish_far_out(prep):
    """Rows whose pre-activations are about +100, -100 and -30 (positive weights, positive and negative rows): swish stays finite and
    correct.  The ordinary rows are held to BAR3 of their own maximum.  Far below zero swish(x) ~ x e^x, so a pre-activation error dx is
    a RELATIVE error |dx| (1 + 1 / |x|) of the result; dx <= BAR3 max|pre| from the GEMM, plus the fp32 rounding of the exponent's
    argument, |x| log2(e) 2^-24 ln 2 <= 1.5e-5 for |x| <= 250.  Below 1e-30 (x < -75: fp32 runs out of exponent near x = -90) only
    the size is asserted."""
    g = R.gen(1800)
    M, N, K = 9, 72, 40
    w = R.weight_for(N, K).abs()
    a = torch.randn(M, K, generator=g)
    p = a[3].abs()
    p = p * (100.0 / (p.double() @ w.double().T).mean().item())
    a[3], a[5], a[7] = p, -p, -0.3 * p
    c = dict(srcs=[a], idxs=[None], widths=[K], w=w, bias=R.vec(N, g, 0.1), kscale=None, kshift=None, M=M, N=N, K=K)
    pre, ref = R.gather_ref(c, 0), R.gather_ref(c, 2)
    assert abs(pre[3].mean() - 100) < 1 and abs(pre[5].mean() + 100) < 1 and 20 < pre[3].min() and pre[3].max() < 250 and pre[7].max() < -7.5
    got = run_gather(c, prep.hilo(N, K, w, "abs"), 2)
    assert torch.isfinite(got).all()
    R.assert_close(got, ref, R.BAR3, "swish, all rows")
    rows = [r for r in range(M) if r not in (3, 5, 7)]
    err = R.assert_close(got[rows], ref[rows], R.BAR3, "swish, ordinary rows")
    print(f"ERR gather_gemm swish ordinary rows {err:.3e} / {R.BAR3:.1e}")
    neg_ref, neg = ref[[5, 7]], got[[5, 7]].double()
    big = neg_ref.abs() > 1e-30
    assert big.sum() >= N and (~big).sum() >= N // 2, "the -30 row is in range, most of the -100 row is not"
    rel = ((neg - neg_ref) / neg_ref).abs()[big].max().item()
    bound = R.BAR3 * pre.abs().max().item() * (1 + 1 / 7.5) + 1.5e-5
    print(f"ERR gather_gemm swish far below zero, relative {rel:.3e} / {bound:.3e}")
    assert rel <= bound and (neg[~big].abs() <= 1e-30).all()


# ---- skgc_layer_norm -------------------------------------------------------------------------------------------------------------------- #
LN_MODES = ["res-absent", "res=out", "x=out", "distinct"]


def run_ln(x, gamma, beta, res, mode):
    rows, N = x.shape
    n = rows * N
    out = _nan(n + SPARE * N)
    xd, rd = _d(x), None
    if mode == "res=out":
        out[:n] = _d(res).flatten()
        rd = out
    elif mode == "x=out":
        out[:n] = xd.flatten()
        xd = out
    elif mode == "distinct":
        rd = _d(res)
    _hip().gc_layer_norm(xd, _d(gamma), _d(beta), rd, out, rows, N)
    return out


def _ln_ref(x, gamma, beta, res, mode):
    return R.layer_norm_ref(x, gamma, beta, res if mode in ("res=out", "distinct") else None)


LN_N = [8, 63, 64, 65, 72, 512, 1000, 1024]
LN_ROWS = [1, 3, 4, 5, 1001]


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("N", LN_N)
def test_layer_norm_ordinary_rows(N, rows):
    """Unit-normal rows, gamma ~ 1; the aliasing mode changes from case to case (all four at N = 65 and N = 1000)."""
    x, gamma, beta, res = R.ln_case("ordinary", rows, N, 100 + N + rows)
    modes = LN_MODES if N in (65, 1000) else [LN_MODES[(LN_N.index(N) + LN_ROWS.index(rows)) % 4]]
    for mode in modes:
        got = _take(run_ln(x, gamma, beta, res, mode), rows, N)
        err = R.assert_close(got, _ln_ref(x, gamma, beta, res, mode), R.BAR3, f"layer_norm N={N} rows={rows} {mode}")
        print(f"ERR layer_norm ordinary N={N} rows={rows} {mode} {err:.3e} / {R.BAR3:.1e}")


@pytest.mark.parametrize("mode", LN_MODES)
@pytest.mark.parametrize("N", LN_N)
def test_layer_norm_offset_and_constant_rows(N, mode):
    """Rows of mean 1e4 and spread 1, and a constant row.  Bound: four times the error of the same two-pass formula in fp32 on the CPU
    against float64 on these inputs (R.LN_OFFSET_FP32: 1.2e-4 .. 3.6e-4, the rounding of the fp32 mean); the constant row is exact."""
    x, gamma, beta, res = R.ln_case("offset", 5, N, 100 + N)
    with_res = mode in ("res=out", "distinct")
    got = _take(run_ln(x, gamma, beta, res, mode), 5, N)
    bound = R.ln_offset_bound(N, with_res)
    err = R.assert_close(got, _ln_ref(x, gamma, beta, res, mode), bound, f"layer_norm offset rows N={N} {mode}")
    print(f"ERR layer_norm offset N={N} {mode} {err:.3e} / {bound:.3e} (fp32 on the CPU: {R.LN_OFFSET_FP32[N][with_res]:.3e})")
    assert torch.equal(got[2], res[2] + beta if with_res else beta), "a constant row gives exactly beta (+ res)"


def test_layer_norm_refusals():
    x, gamma, beta, res = R.ln_case("ordinary", 4, 1025, 7)
    out = _nan(4 * 1025)
    _refused(lambda: _hip().gc_layer_norm(_d(x), _d(gamma), _d(beta), None, out, 4, 1025), out)
    _refused(lambda: _hip().gc_layer_norm(_d(x), _d(gamma), _d(beta), None, out, 0, 1024), out)
    _refused(lambda: _hip().gc_layer_norm(_d(x), _d(gamma), _d(beta), None, out, 4, 0), out)


# ---- skgc_segment_sum -------------------------------------------------------------------------------------------------------------------- #
def _segments(n_nodes, g):
    """(lead, counts, tail): rows before offsets[0] and after offsets[-1] belong to nobody."""
    if n_nodes == 1:
        return 2, torch.tensor([23]), 3                                    # all edges in one node
    if n_nodes == 4:
        return 1, torch.tensor([0, 5, 1, 0]), 2                            # empty first and last
    if n_nodes == 5:
        return 3, torch.tensor([4, 0, 0, 0, 2]), 1                         # a run of three empty nodes
    counts = torch.randint(1, 7, (n_nodes,), generator=g)
    counts[0] = counts[-1] = 0
    counts[10:13] = 0
    counts[20] = 1000                                                      # one segment of 1000 edges
    return 3, counts, 5


@pytest.mark.parametrize("n_nodes", [1, 4, 5, 50])
@pytest.mark.parametrize("N", [4, 32, 260, 512, 1028])
def test_segment_sum(N, n_nodes):
    g = R.gen(300 + N + n_nodes)
    lead, counts, tail = _segments(n_nodes, g)
    E = lead + int(counts.sum()) + tail
    offsets = (lead + torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])).int()
    assert offsets[0] > 0 and offsets[-1] < E
    e, acc0 = torch.randn(E, N, generator=g), torch.randn(E, N, generator=g)
    ref, _ = R.segment_sum_ref(e, offsets, n_nodes)
    mass, _ = R.segment_sum_ref(e.abs(), offsets, n_nodes)
    ed, od = _d(e), _d(offsets)
    out, acc = _nan((n_nodes + SPARE) * N), _nan(E * N)
    acc[:E * N] = _d(acc0).flatten()
    _hip().gc_segment_sum(ed, od, out, acc, n_nodes, N)
    got = _take(out, n_nodes, N)
    # recursive fp32 summation of len terms: |error| <= (len - 1) 2^-24 sum|e| per element (a run of one is exact)
    bound = (counts - 1).clamp(min=0).double()[:, None] * U * mass
    excess = ((got.double() - ref).abs() - bound).max().item()
    worst = ((got.double() - ref).abs() / bound.clamp_min(1e-300))[counts > 1].max().item() if (counts > 1).any() else 0.0
    print(f"ERR segment_sum N={N} nodes={n_nodes} error / bound {worst:.3e}")
    assert torch.isfinite(got).all() and excess <= 0
    assert (got[counts == 0] == 0).all(), "a node without edges gets zeros"
    a = _take(acc, E, N)
    j0, j1 = int(offsets[0]), int(offsets[-1])
    assert torch.equal(a[j0:j1], (acc0 + e)[j0:j1]), "acc = acc0 + e bit for bit on the covered rows"
    assert torch.equal(a[:j0], acc0[:j0]) and torch.equal(a[j1:], acc0[j1:]), "acc is untouched on rows that belong to nobody"
    out2 = _nan((n_nodes + SPARE) * N)
    _hip().gc_segment_sum(ed, od, out2, None, n_nodes, N)
    assert torch.equal(_take(out2, n_nodes, N), got), "acc = None changes the sums"


def test_segment_sum_refuses_a_width_that_is_no_multiple_of_4():
    e, off = _d(torch.randn(10, 6, generator=R.gen(1))), _d(torch.tensor([0, 4, 10]).int())
    out = _nan(2 * 6)
    _refused(lambda: _hip().gc_segment_sum(e, off, out, None, 2, 6), out)
    _refused(lambda: _hip().gc_segment_sum(e, off, out, None, 0, 8), out)


# ---- skgc_prepare_weight_perm8 + skgc_linear_layer_norm ------------------------------------------------------------------------------------ #
LIN_MODES = ["res-absent", "res=out", "distinct"]


def run_linear(c, P, mode, rows=None):
    planes, plane, ldw = P
    rows = c["a"].shape[0] if rows is None else rows
    out = _nan((rows + SPARE) * L)
    rd = None
    if mode == "res=out":
        out[:rows * L] = _d(c["res"]).flatten()
        rd = out
    elif mode == "distinct":
        rd = _d(c["res"])
    a = _d(c["a"])
    _hip().gc_linear_layer_norm(a, a.shape[1], c["K"], planes, plane, ldw, _d(c["bias"]), _d(c["gamma"]), _d(c["beta"]), rd, out, rows)
    return _take(out, rows, L)


def _lin_ref(c, mode):
    return R.linear_layer_norm_ref(c["a"], c["K"], c["w"], c["bias"], c["gamma"], c["beta"], None if mode == "res-absent" else c["res"])


LIN_K = [8, 24, 32, 40, 512, 520]
LIN_ROWS = [1, 127, 128, 129, 300]


@pytest.mark.parametrize("rows", LIN_ROWS)
@pytest.mark.parametrize("K", LIN_K)
def test_linear_layer_norm_k_and_row_tails(prep, K, rows):
    """lda = K + 4 (aligned rows) or K + 3 (three rows in four misaligned: the loader's element-wise branch), by case; an all-zero row
    of a where there are three rows or more; the residual mode changes from case to case (all three at K = 40)."""
    i = LIN_K.index(K) + LIN_ROWS.index(rows)
    c = R.linear_case(K, rows, seed=3000 + K + rows, lda_pad=4 if i % 2 == 0 else 3)
    for mode in (LIN_MODES if K == 40 else [LIN_MODES[i % 3]]):
        err = R.assert_close(run_linear(c, prep.perm8(K), mode), _lin_ref(c, mode), R.BAR_LN, f"linear_layer_norm K={K} rows={rows} {mode}")
        print(f"ERR linear_layer_norm K={K} rows={rows} {mode} {err:.3e} / {R.BAR_LN:.1e}")


@pytest.mark.parametrize("mode", LIN_MODES)
@pytest.mark.parametrize("K", [8, 40, 512])
def test_linear_layer_norm_offset_rows_and_the_zero_row(prep, K, mode):
    """A bias of 50 on every column: the pre-norm rows are offset, and the all-zero row of a is constant before the norm (every partial
    sum of 512 fifties is an fp32 integer: the mean is exact), so it comes out as exactly beta (+ res)."""
    c = R.linear_case(K, 129, seed=3100 + K, bias50=True)
    got = run_linear(c, prep.perm8(K), mode)
    err = R.assert_close(got, _lin_ref(c, mode), R.BAR_LN, f"linear_layer_norm bias 50 K={K} {mode}")
    print(f"ERR linear_layer_norm bias50 K={K} {mode} {err:.3e} / {R.BAR_LN:.1e}")
    z = 129 // 2
    assert not c["a"][z].any()
    assert torch.equal(got[z], c["beta"] if mode == "res-absent" else c["res"][z] + c["beta"]), "the zero row gives exactly beta (+ res)"


def test_linear_layer_norm_identity_weight_shows_the_column_order(prep):
    c = dict(R.identity_case(129, seed=5000), K=L, res=None)
    got = run_linear(c, prep.perm8(L, c["w"], "eye"), "res-absent")
    ref = R.layer_norm_ref(c["a"], c["gamma"], c["beta"])
    err = R.assert_close(got, ref, R.BAR_LN, "linear_layer_norm W = I")
    print(f"ERR linear_layer_norm identity {err:.3e} / {R.BAR_LN:.1e}")


def test_prepare_weight_perm8_and_linear_layer_norm_refusals(prep):
    lib, st = _lib(), _stream()
    w = _d(R.weight_for(L, 40))
    dst = torch.full((2 * L * 48 + MARGIN,), float("nan"), dtype=torch.float16, device=DEV)
    small = _d(R.weight_for(L, 40)[:500])
    for args in ((small, 500, 40, L * 40, 40),           # N = 500: no multiple of 32
                 (w, L, 40, L * 40, 32),                 # ldw < K
                 (w, L, 40, L * 44, 44),                 # ldw % 8 != 0
                 (w, L, 40, L * 40 - 8, 40),             # a plane smaller than N ldw
                 (w, L, 0, L * 40, 40)):                 # K = 0
        src, N, K, plane, ldw = args
        assert lib.skgc_prepare_weight_perm8(src.data_ptr(), N, K, dst.data_ptr(), plane, ldw, st) == -1, args[1:]
    torch.cuda.synchronize()
    assert _all_nan(dst)
    c = R.linear_case(40, 5, seed=3200)
    planes, plane, ldw = prep.perm8(40)
    a, out = _d(c["a"]), _nan(5 * L)
    tail = (_d(c["bias"]), _d(c["gamma"]), _d(c["beta"]), None, out, 5)
    _refused(lambda: _hip().gc_linear_layer_norm(a, 39, 40, planes, plane, ldw, *tail), out)               # lda < K
    _refused(lambda: _hip().gc_linear_layer_norm(a, 44, 40, planes, plane, 32, *tail), out)                # ldw < K
    _refused(lambda: _hip().gc_linear_layer_norm(a, 44, 36, planes, plane, 36, *tail), out)                # ldw % 8 != 0
    _refused(lambda: _hip().gc_linear_layer_norm(a, 44, 40, planes, plane, ldw, *tail[:-1], 0), out)       # rows = 0


# ---- skgc_sum_linear_layer_norm ------------------------------------------------------------------------------------------------------------- #
def run_sum(c, P, act, mode, group, bias=True, rows=None, srcs=None, offs=None, lds=None, idxs=None, K=None, out=None):
    planes, plane, ldw = P
    rows = c["rows"] if rows is None else rows
    n = len(c["bufs"])
    out = _nan((rows + SPARE) * L) if out is None else out
    rd = None
    if mode == "res=out":
        out[:rows * L] = _d(c["res"]).flatten()
        rd = out
    elif mode == "distinct":
        rd = _d(c["res"])
    _hip().gc_sum_linear_layer_norm([_d(b) for b in c["bufs"]] if srcs is None else srcs, [c["off"]] * n if offs is None else offs,
                                    [c["ld"]] * n if lds is None else lds, [_d(i) for i in c["idxs"]] if idxs is None else idxs,
                                    c["K"] if K is None else K, act, planes, plane, ldw, _d(c["bias"]) if bias else None, _d(c["gamma"]), _d(c["beta"]),
                                    rd, out, rows, group)
    return _take(out, rows, L)


# (n_src, index arrays, K, act, bias, residual, rows)
SUM_CASES = [
    (1, (None,), 8, 0, True, "res-absent", 1),
    (1, ("rand",), 40, 2, False, "res=out", 128),
    (2, (None, "rand"), 512, 2, True, "distinct", 129),
    (2, ("rand", "rand"), 8, 2, True, "res=out", 300),
    (2, (None, None), 40, 0, False, "res-absent", 129),
    (3, (None, "rand", "rand"), 512, 2, True, "res=out", 300),
    (3, ("rand", "repeat", "last"), 40, 2, True, "distinct", 128),
    (3, (None, None, None), 8, 0, True, "res-absent", 129),
    (3, ("rand", None, "rand"), 512, 0, False, "distinct", 1),
    (3, (None, "rand", "rand"), 40, 2, False, "res-absent", 300),
]


@pytest.mark.parametrize("case", SUM_CASES, ids=[f"{c[0]}src-K{c[2]}-act{c[3]}-{c[5]}-rows{c[6]}-{i}" for i, c in enumerate(SUM_CASES)])
def test_sum_linear_layer_norm_group_0_and_1(prep, case):
    """One to three sources with index arrays on none, some and all of them, read from element offset 4 of rows with ld = K + 8; group 0
    and group 1 are the same kernel: the same bits."""
    n_src, kinds, K, act, bias, mode, rows = case
    c = R.sum_case(n_src, kinds, K, rows, seed=6000 + SUM_CASES.index(case))
    ref = R.sum_linear_layer_norm_ref(c["views"], c["idxs"], K, act, c["w"], c["bias"] if bias else None, c["gamma"], c["beta"],
                                      None if mode == "res-absent" else c["res"], rows)
    got = run_sum(c, prep.perm8(K), act, mode, 0, bias)
    err = R.assert_close(got, ref, R.BAR_LN, f"sum_linear_layer_norm {case}")
    print(f"ERR sum_linear_layer_norm {case} {err:.3e} / {R.BAR_LN:.1e}")
    assert torch.equal(run_sum(c, prep.perm8(K), act, mode, 1, bias), got), "group 0 and group 1 differ"


@pytest.mark.parametrize("G,K", [(1, 40), (15, 8), (16, 512), (17, 40), (37, 512)])
def test_sum_linear_layer_norm_group_of_three(prep, G, K):
    """The index entries of the padding groups (>= G) point at rows filled with 1e30: nothing of them reaches an output."""
    c = R.group3_case(G, K, seed=4000 + G)
    planes, plane, ldw = prep.perm8(K)
    out = _nan((G + SPARE) * L)
    _hip().gc_sum_linear_layer_norm([_d(s) for s in c["srcs"]], [0, 0, 0], [K, K, K], [_d(i) for i in c["idxs"]], K, 2, planes, plane, ldw,
                                    _d(c["bias"]), _d(c["gamma"]), _d(c["beta"]), None, out, G, 3)
    err = R.assert_close(_take(out, G, L), R.group3_ref(c), R.BAR_LN, f"sum_linear_layer_norm group 3 G={G}")
    print(f"ERR sum_linear_layer_norm group3 G={G} K={K} {err:.3e} / {R.BAR_LN:.1e}")


def test_sum_linear_layer_norm_is_the_edge_mlp_by_distributivity(prep):
    """fc1(concat(e, v_s[send], v_r[recv])) = e W_e^T + b1 + (v_s W_s^T)[send] + (v_r W_r^T)[recv]: skgc_sum_linear_layer_norm on the
    three precomputed terms against skgc_gather_gemm over the concatenation + skgc_linear_layer_norm, and both against float64."""
    g = R.gen(7000)
    rows, ns, nr = 130, 20, 10
    e, vs, vr = torch.randn(rows, L, generator=g), torch.randn(ns, L, generator=g), torch.randn(nr, L, generator=g)
    send, recv = R.index(ns, rows, g), R.index(nr, rows, g)
    w1, b1 = R.weight_for(L, 3 * L), R.vec(L, g)
    c2 = R.linear_case(L, rows, seed=7001, lda_pad=0)
    w2, b2, gam, bet, res = c2["w"], c2["bias"], c2["gamma"], c2["beta"], c2["res"]
    h64 = R.gather_gemm_ref([e, vs, vr], [None, send, recv], [L, L, L], w1, b1, 2)
    ref = R.linear_layer_norm_ref(h64, L, w2, b2, gam, bet, res)
    hip, P = _hip(), prep.perm8(L)
    # the two kernels it replaces
    W1 = prep.hilo(L, 3 * L)
    h = torch.full((rows, L), float("nan"), device=DEV)
    hip.gc_gather_gemm([_d(e), _d(vs), _d(vr)], [None, _d(send), _d(recv)], [L, L, L], W1.buf, W1.plane, W1.ldw, _d(b1), h, rows, L, 2, None, None)
    two = run_linear(dict(a=h.cpu(), K=L, bias=b2, gamma=gam, beta=bet, res=res), P, "distinct")
    # the three terms (each Linear by the same GEMM, without activation), then the sum kernel
    terms = []
    for s, (x, bias) in enumerate(((e, b1), (vs, torch.zeros(L)), (vr, torch.zeros(L)))):
        Ws = prep.hilo(L, L, w1[:, s * L:(s + 1) * L].contiguous(), f"w1[{s}]")
        t = torch.full((x.shape[0], L), float("nan"), device=DEV)
        hip.gc_gather_gemm([_d(x)], [None], [L], Ws.buf, Ws.plane, Ws.ldw, _d(bias), t, x.shape[0], L, 0, None, None)
        terms.append(t)
    out = _nan((rows + SPARE) * L)
    hip.gc_sum_linear_layer_norm(terms, [0, 0, 0], [L, L, L], [None, _d(send), _d(recv)], L, 2, *P, _d(b2), _d(gam), _d(bet), _d(res), out, rows, 0)
    one = _take(out, rows, L)
    e1 = R.assert_close(one, ref, R.BAR_LN, "three terms + sum kernel against float64")
    e2 = R.assert_close(two, ref, R.BAR_LN, "gather_gemm + linear_layer_norm against float64")
    e3 = R.assert_close(one, two, R.BAR_LN, "the sum kernel against the two kernels it replaces")
    print(f"ERR distributivity sum-kernel {e1:.3e} two-kernels {e2:.3e} each-other {e3:.3e} / {R.BAR_LN:.1e}")


def test_sum_linear_layer_norm_refusals(prep):
    from skyrim_amd.graphcast.engine import SumDesc
    c = R.sum_case(3, ("rand", "rand", "rand"), 40, 5, seed=6100)
    P = prep.perm8(40)
    out = _nan((5 + SPARE) * L)
    bufs, ix = [_d(b) for b in c["bufs"]], [_d(i) for i in c["idxs"]]
    call = lambda **kw: (lambda: run_sum(c, P, kw.pop("act", 2), kw.pop("mode", "res-absent"), kw.pop("group", 0), out=out, srcs=bufs, **kw))  # noqa: E731
    _refused(call(K=36), out)                                   # K % 8 != 0
    _refused(call(lds=[48, 46, 48]), out)                       # ld % 4 != 0
    _refused(call(lds=[48, 36, 48]), out)                       # ld < K
    _refused(call(offs=[4, 1, 4]), out)                         # a source pointer off by one float: not 16-byte aligned
    _refused(call(group=2), out)
    _refused(call(act=1), out)
    _refused(call(group=3, idxs=[ix[0], None, ix[2]], rows=1), out)      # group 3 needs every index array (never launched: the arrays are not in virtual order)
    # group 3 with a residual: the index arrays of a real group-of-three case
    g3 = R.group3_case(5, 40, seed=4005)
    res = _d(torch.zeros(5, L))
    _refused(lambda: _hip().gc_sum_linear_layer_norm([_d(s) for s in g3["srcs"]], [0, 0, 0], [40, 40, 40], [_d(i) for i in g3["idxs"]], 40, 2, *P,
                                                     _d(g3["bias"]), _d(g3["gamma"]), _d(g3["beta"]), res, out, 5, 3), out)
    # n_src 0 and 4: the op refuses them itself, so these go to the library
    keep = [_d(c["gamma"]), _d(c["beta"])]
    for n_src in (0, 4):
        d = SumDesc()
        for s in range(3):
            d.src[s], d.idx[s], d.ld[s] = bufs[s].data_ptr(), ix[s].data_ptr(), c["ld"]
        d.n_src, d.K, d.act = n_src, 40, 2
        d.w, d.w_plane, d.ldw = P[0].data_ptr(), P[1], P[2]
        d.gamma, d.beta, d.out, d.rows, d.group = keep[0].data_ptr(), keep[1].data_ptr(), out.data_ptr(), 5, 0
        assert _lib().skgc_sum_linear_layer_norm(ctypes.byref(d), _stream()) == -1
    torch.cuda.synchronize()
    assert _all_nan(out)
