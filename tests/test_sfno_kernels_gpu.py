"""SFNO building blocks of include/skyrim_sfno.h at their edges, each against a float64 restatement written here: sksfno_gemm_run over
every dispatch branch of its launcher (A loader / precision, tile, epilogue order), ragged batches (k_lo_step, m_cap), the XCD re-map of
the workgroups, the loader's per-k affine and second source; sksfno_instance_norm and sksfno_instance_stats at odd sizes, large offsets
and far outliers.  Outputs start as a NaN sentinel, so an element that is never written shows, and so does one written twice where the
output aliases res_post."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1 << 30                  # "no split" value of the two-level row index
BAR3 = 2e-6                    # 3-term fp16 hi/lo products: max|err| / max|ref|
# terms = 2 rounds A to one fp16 plane (round to nearest: relative error <= 2^-11 per element); W keeps hi/lo.  Bound per output element:
# 2^-11 sum_k |A W| (GELU's slope is <= 1.13, swish's <= 1.1: x 1.2), plus the 3-term bar for what the W planes and fp32 accumulation add.
BAR2_A = 1.2 * 2.0 ** -11


def _lib():
    from skyrim_amd.sfno import engine
    return engine.load_library()


def _weight(w: torch.Tensor):
    from skyrim_amd import native
    lib = _lib()
    return native.HiLoWeight(torch.device(DEV), lib.sksfno_prepare_weight, w)


def branch(*, M, N, K, a_off, a_sb, a_m1, a_sm, a_sm2, a_sk, o_sm, o_sn, terms, affine, two_sources):
    """The launcher's dispatch (sfno_ops.hip: sksfno_gemm_run), restated: (loader, tile, swap).  Keep in sync with the `fast`, `vec`, `swap`
    and `wide` predicates there: the cases below assert the branch they are meant for through this copy.  ``a`` comes from the caching allocator
    (256-byte aligned), so its address is 16-byte aligned exactly when a_off is a multiple of 4."""
    extent = ((M - 1) // a_m1) * a_sm2 + (min(a_m1, M) - 1) * a_sm + (K - 1) * a_sk
    fast = terms != 2 and not affine and not two_sources and K % 8 == 0 and a_sm >= 0 and a_sm2 >= 0 and a_sk > 0 and extent < (1 << 30)
    vec = fast and a_sk == 1 and a_off % 4 == 0 and a_sm % 4 == 0 and a_sm2 % 4 == 0 and a_sb % 4 == 0
    loader = "vec" if vec else "fast" if fast else "x2w" if terms == 2 else "x3"
    swap = not (o_sm == 1 and o_sn != 1)
    wide = not swap and 128 < N <= 256
    return loader, "TG" if wide else "TS", swap


def _index(B, M, X, off, sb, m1, sm, sm2, sx):
    """Flat element index [B][M][X] of the two-level row addressing: off + b sb + (m / m1) sm2 + (m % m1) sm + x sx."""
    b = torch.arange(B)[:, None, None]
    m = torch.arange(M)[None, :, None]
    x = torch.arange(X)[None, None, :]
    return off + b * sb + (m // m1) * sm2 + (m % m1) * sm + x * sx


def _act(v, act):
    if act == 1:
        return torch.nn.functional.gelu(v)
    if act == 2:
        return v * torch.sigmoid(v)
    return v


def run_gemm(*, M, N, K, batch=1, a_off=0, a_sb=0, a_m1=BIG, a_sm, a_sm2=0, a_sk, o_off=0, o_sb=0, o_m1=BIG, o_sm, o_sm2=0, o_sn,
             act=0, bias=False, res_pre=False, res_post=False, alias=False, k_lo_step=0, m_cap0=0, m_cap_step=0, terms=3,
             affine=None, a2=None, a2_k_split=0, seed=0, a_gen=None, w_batched=None):
    """One sfno_gemm call on random data; returns (got, ref, written, untouched_ok, |A||W| bound, branch) with got / ref over the written
    elements.  ``affine``: (scale, shift) per k; ``a2``: the k stride of a second source (K-concatenation at a2_k_split)."""
    gen = torch.Generator().manual_seed(seed)
    ia = _index(batch, M, K, a_off, a_sb, a_m1, a_sm, a_sm2, a_sk)
    io = _index(batch, M, N, o_off, o_sb, o_m1, o_sm, o_sm2, o_sn)
    if a2 is not None:                               # k >= split from the second source: same rows, k stride a2
        ia2 = _index(batch, M, K, 0, 0, a_m1, a_sm, a_sm2, a2) - a2 * a2_k_split
        n_a2 = int(ia2[..., a2_k_split:].max()) + 1
    n_a, n_o = int(ia.max()) + 1 + 7, int(io.max()) + 1 + 7
    a = (a_gen(n_a, gen) if a_gen else torch.randn(n_a, generator=gen)).float()
    wb = batch if (batch > 1 if w_batched is None else w_batched) else 1
    w = torch.randn(wb, N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen) if bias else None
    rp = torch.randn(n_o, generator=gen) if res_pre else None
    rq = torch.randn(n_o, generator=gen) if (res_post or alias) else None
    A = a.double()[ia]                                # [B][M][K]
    if a2 is not None:
        a2v = (a_gen(n_a2, gen) if a_gen else torch.randn(n_a2, generator=gen)).float()
        A[..., a2_k_split:] = a2v.double()[ia2[..., a2_k_split:]]
    if affine is not None:
        A = A * affine[0].double() + affine[1].double()
    kk = torch.arange(K)
    kb = [(bb * k_lo_step) // 32 * 32 for bb in range(batch)]
    mask_k = torch.stack([(kk >= kb[bb]).double() for bb in range(batch)])[:, None, :]       # [B][1][K]
    Wd = w.double().expand(batch, N, K)
    ref = torch.einsum("bmk,bnk->bmn", A * mask_k, Wd)
    bound = torch.einsum("bmk,bnk->bmn", (A * mask_k).abs(), Wd.abs())
    if b is not None:
        ref = ref + b.double()
    if rp is not None:
        ref = ref + rp.double()[io]
    ref = _act(ref, act)
    if rq is not None:
        ref = ref + rq.double()[io]
    rows = torch.full((batch,), M) if m_cap_step <= 0 else torch.tensor([min(M, m_cap0 + bb * m_cap_step) for bb in range(batch)])
    written = torch.arange(M)[None, :, None] < rows[:, None, None]                           # [B][M][1]
    written = written.expand(batch, M, N)
    # the output buffer: NaN everywhere, res_post's values where the output aliases it
    out0 = torch.full((n_o,), float("nan"))
    if alias:
        out0[io.reshape(-1)] = rq[io.reshape(-1)]
    outd = out0.to(DEV)
    W = _weight(w)
    geom = [a_off, a_sb, a_m1, a_sm, a_sm2, a_sk, W.w_sb if wb > 1 else 0, W.plane, W.ldw, o_off, o_sb, o_m1, o_sm, o_sm2, o_sn,
            M, N, K, batch, act, k_lo_step, m_cap0, m_cap_step, a2 or 0, a2_k_split, terms]
    dv = lambda t: None if t is None else t.float().contiguous().to(DEV)  # noqa: E731
    torch.ops.skyrim_hip.sfno_gemm(a.to(DEV), W.buf, outd, dv(b), dv(rp), outd if alias else dv(rq),
                                   dv(affine[0]) if affine else None, dv(affine[1]) if affine else None,
                                   dv(a2v) if a2 is not None else None, geom)
    out = outd.cpu()
    got = out.double()[io]
    # every element outside the written set keeps its start value bit for bit (NaN sentinel or the aliased residual)
    keep = torch.ones(n_o, dtype=torch.bool)
    keep[io[written].reshape(-1)] = False
    untouched = torch.equal(out.view(torch.int32)[keep], out0.view(torch.int32)[keep])
    br = branch(M=M, N=N, K=K, a_off=a_off, a_sb=a_sb, a_m1=a_m1, a_sm=a_sm, a_sm2=a_sm2, a_sk=a_sk, o_sm=o_sm, o_sn=o_sn, terms=terms,
                affine=affine is not None, two_sources=a2 is not None)
    return got, ref, written, untouched, bound, br


def _rel(got, ref, written):
    g, r = got[written], ref[written]
    return ((g - r).abs().max() / r.abs().max()).item()


# ---- 1. the dispatch matrix ----------------------------------------------------------------------------------------------------- #
# (id, expected branch, arguments).  Layouts: "rows" = A [M][K] row-major (k contiguous), "nchw" = A [K][M] (rows contiguous);
# output "cm" = [N][M] (rows contiguous: un-swapped), "rm" = [M][N] (columns contiguous: swapped).
GEMM_CASES = [
    ("vec-TS-N1", ("vec", "TS", False),
     dict(M=200, N=1, K=40, a_sm=40, a_sk=1, o_sm=1, o_sn=200, act=0, bias=True)),
    ("vec-TG", ("vec", "TG", False),
     dict(M=130, N=200, K=72, a_sm=72, a_sk=1, o_sm=1, o_sn=130, act=2, bias=True, res_pre=True)),
    ("vec-TS-swap-alias", ("vec", "TS", True),
     dict(M=150, N=29, K=64, a_sm=64, a_sk=1, o_sm=29, o_sn=1, act=1, bias=True, alias=True)),
    ("fast-misaligned-swap-N130", ("fast", "TS", True),
     dict(M=129, N=130, K=48, a_off=1, a_sm=48, a_sk=1, o_sm=130, o_sn=1, act=2, res_post=True)),
    ("fast-nchw-batched", ("fast", "TS", False),
     dict(M=300, N=64, K=24, batch=2, a_sb=300 * 24, a_sm=1, a_sk=300, o_sb=64 * 300, o_sm=1, o_sn=300, act=1, bias=True, res_pre=True,
          res_post=True)),
    ("fast-nchw-TG", ("fast", "TG", False),
     dict(M=257, N=256, K=8, a_sm=1, a_sk=257, o_sm=1, o_sn=257, act=0, res_post=True)),
    ("x3-two-level-Ktail", ("x3", "TS", False),
     dict(M=74, N=29, K=45, batch=3, a_sb=37 * 45 * 2, a_m1=2, a_sm=1, a_sm2=45 * 2, a_sk=2, o_sb=29 * 74, o_m1=2, o_sm=1, o_sm2=2,
          o_sn=74, act=1, bias=True, res_pre=True, res_post=True)),
    ("x3-swap-Ktail-N1", ("x3", "TS", True),
     dict(M=131, N=1, K=13, a_sm=13, a_sk=1, o_sm=1, o_sn=1, act=2, bias=True)),
    ("x2w-TG", ("x2w", "TG", False),
     dict(M=100, N=160, K=64, a_sm=64, a_sk=1, o_sm=1, o_sn=100, act=0, bias=True, terms=2)),
    ("x2w-swap-Ktail", ("x2w", "TS", True),
     dict(M=140, N=40, K=44, a_sm=1, a_sk=140, o_sm=40, o_sn=1, act=1, res_pre=True, alias=True, terms=2)),
]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_dispatch_matrix_against_float64(case):
    _, want, kw = case
    got, ref, written, untouched, bound, br = run_gemm(seed=len(kw) * 7 + kw["K"], **kw)
    assert br == want, f"launcher branch {br}, the case is meant for {want}"
    assert untouched, "an element outside the output was written"
    assert torch.isfinite(got[written]).all(), "an output element was not written"
    if kw.get("terms", 3) == 2:
        err = (got - ref).abs()[written]
        lim = (BAR2_A * bound + BAR3 * ref.abs().max())[written]
        assert (err <= lim).all(), f"terms=2: worst err / bound {(err / lim).max().item():.3f}"
        assert _rel(got, ref, written) > 1e-6          # the fp16 rounding of A is really there: this is not the 3-term path
    else:
        assert _rel(got, ref, written) < BAR3


def test_dispatch_matrix_covers_every_branch():
    seen = {c[1] for c in GEMM_CASES}
    assert {b[0] for b in seen} == {"vec", "fast", "x2w", "x3"}
    assert {b[1] for b in seen} == {"TS", "TG"} and {b[2] for b in seen} == {True, False}
    assert {c[2].get("act") for c in GEMM_CASES} == {0, 1, 2}
    assert any(c[2]["N"] == 1 for c in GEMM_CASES) and any(c[2]["K"] % 32 and c[2]["K"] % 8 == 0 for c in GEMM_CASES)
    assert any(c[2]["M"] % 128 for c in GEMM_CASES) and any(c[2].get("alias") for c in GEMM_CASES)
    assert any(c[2].get("a_off", 0) % 4 and c[1][0] == "fast" for c in GEMM_CASES)


# ---- 2. ragged batches --------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("K,layout", [(96, "rows"), (100, "rows"), (96, "nchw"), (65, "nchw")])
def test_k_lo_step_contracts_from_the_32_aligned_floor(K, layout):
    """Batch b contracts k >= floor32(b k_lo_step) only: the A entries below are random (not zero), so a kernel that reads them fails.
    k_lo_step 20 over 5 batches: floors 0, 0, 32, 32, 64 -- the contraction start crosses 32 and 64.  K = 65: the last batch of
    k_lo_step 32 contracts one k."""
    M, N, B = 70, 48, 5
    step = 20 if K != 65 else 32
    B = B if K != 65 else 3
    if layout == "rows":          # A[b] [M][K]
        kw = dict(a_sb=M * K, a_sm=K, a_sk=1)
    else:                         # the synthesis' layout: rows contiguous, k strided
        kw = dict(a_sb=M, a_sm=1, a_sk=B * M)
    got, ref, written, untouched, _, br = run_gemm(M=M, N=N, K=K, batch=B, **kw, o_sb=M * N, o_sm=1, o_sn=M, act=1, bias=True,
                                                   k_lo_step=step, seed=K)
    assert br[0] == ("vec" if layout == "rows" and K % 8 == 0 else "fast" if K % 8 == 0 else "x3")
    assert untouched and torch.isfinite(got).all()
    assert _rel(got, ref, written) < BAR3


@pytest.mark.parametrize("K", [64, 45])
def test_m_cap_leaves_rows_at_or_above_the_cap_untouched(K):
    """Batch b computes rows m < m_cap0 + b m_cap_step: caps 0 (m_cap0 = 0: nothing), 70 (inside the first 128-row tile), 140 and 210
    (inside the second), 280 (inside the third, ragged one), 350 (above M = 300: every row).  Rows at or above a cap keep the NaN
    sentinel bit for bit."""
    M, N, B = 300, 40, 6
    got, ref, written, untouched, _, br = run_gemm(M=M, N=N, K=K, batch=B, a_sb=M * K, a_sm=K, a_sk=1, o_sb=M * N, o_sm=N, o_sn=1,
                                                   bias=True, m_cap0=0, m_cap_step=70, seed=K + 1)
    assert br[0] == ("vec" if K == 64 else "x3")
    assert untouched, "a row at or above its batch's m_cap was written"
    assert not written[0].any() and written[-1].all()
    assert torch.isfinite(got[written]).all()
    assert _rel(got, ref, written) < BAR3


def test_empty_contraction_batch_is_refused():
    """floor32((batch - 1) k_lo_step) >= K leaves the last batch nothing to contract: the launcher refuses the descriptor
    (SKSFNO_E_ARG) instead of leaving that batch's output unwritten."""
    with pytest.raises(RuntimeError, match="invalid argument"):
        run_gemm(M=40, N=16, K=40, batch=3, a_sb=40 * 40, a_sm=40, a_sk=1, o_sb=40 * 16, o_sm=1, o_sn=40, k_lo_step=32)
    with pytest.raises(RuntimeError, match="invalid argument"):            # strided loader, K not a multiple of 8
        run_gemm(M=40, N=16, K=63, batch=3, a_sb=40, a_sm=1, a_sk=120, o_sb=40 * 16, o_sm=1, o_sn=40, k_lo_step=32)


# ---- 3. the XCD re-map of the workgroups --------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("gx,gy,batch", [(1, 1, 1), (2, 1, 1), (3, 1, 2), (1, 4, 1), (5, 1, 1), (3, 2, 1), (7, 1, 1), (3, 3, 1),
                                         (5, 3, 1), (23, 1, 1), (1, 23, 1)])
def test_every_tile_is_written_once(gx, gy, batch):
    """T = gx gy tiles of 128 x 128 (TS, swapped order) per batch entry: T = 1..7 and T mod 8 in {1, 7} (9, 15, 23).  The output
    aliases res_post, so a tile written twice adds the residual twice; a tile never written keeps it (and fails the comparison)."""
    M, N = 128 * gy - 5, 128 * gx - 3
    got, ref, written, untouched, _, br = run_gemm(M=M, N=N, K=24, batch=batch, a_sb=M * 24, a_sm=24, a_sk=1, o_sb=M * N, o_sm=N, o_sn=1,
                                                   alias=True, seed=gx * 31 + gy)
    assert br == ("vec", "TS", True)
    assert untouched and _rel(got, ref, written) < BAR3


# ---- 4. the loader's per-k affine and second source ----------------------------------------------------------------------------- #
BAR_AFFINE = 3e-6     # inputs ~1e4: x * scale + shift in fp32 is good to half an ulp of ~33 (1.9e-6 of the unit-variance result) per element


def _raw(n, gen):
    return 1e4 + 300 * torch.randn(n, generator=gen)           # raw fields outside the fp16 range


@pytest.mark.parametrize("layout", ["nchw", "rows"])
def test_per_k_affine_normalises_before_the_split(layout):
    M, N, K = 500, 40, 20
    kw = dict(a_sm=1, a_sk=M) if layout == "nchw" else dict(a_sm=K, a_sk=1)
    scale = torch.full((K,), 1 / 300.0) * (1 + 0.1 * torch.arange(K) / K)
    shift = -1e4 * scale
    got, ref, written, untouched, _, br = run_gemm(M=M, N=N, K=K, **kw, o_sm=1, o_sn=M, act=1, bias=True, affine=(scale, shift), a_gen=_raw)
    assert br[0] == "x3"
    assert untouched and _rel(got, ref, written) < BAR_AFFINE


@pytest.mark.parametrize("split", [8, 32])
def test_second_source_along_k(split):
    """concat(features, normalised raw state) along K (the un-fused decoder): a2_k_split at 8 and at K - 8."""
    M, N, K = 300, 24, 40
    scale = torch.cat([torch.ones(split), torch.full((K - split,), 1 / 300.0)])
    shift = torch.cat([torch.zeros(split), torch.full((K - split,), -1e4 / 300.0)])

    def mixed(n, g):                 # a: features ~N(0, 1) in the first call, the raw state ~1e4 in the second
        mixed.calls += 1
        return torch.randn(n, generator=g) if mixed.calls == 1 else _raw(n, g)
    mixed.calls = 0
    got, ref, written, untouched, _, br = run_gemm(M=M, N=N, K=K, a_sm=1, a_sk=M, o_sm=1, o_sn=M, act=1, bias=True, res_post=True,
                                                   affine=(scale, shift), a2=M, a2_k_split=split, a_gen=mixed, seed=split)
    assert br[0] == "x3"
    assert untouched and _rel(got, ref, written) < BAR_AFFINE


# ---- 5. instance norm and its statistics ----------------------------------------------------------------------------------------- #
EPS = 1e-6
OUTLIER_HW = 721 * 1440


def _norm_input(C, HW, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(C, HW, generator=gen, dtype=torch.float64)
    if kind == "plain":
        x = x * torch.linspace(0.5, 3, C, dtype=torch.float64)[:, None] + torch.linspace(-2, 2, C, dtype=torch.float64)[:, None]
    elif kind == "offset":                    # a large common offset: 1e4 +- 1
        x = x + 1e4
    elif kind.startswith("outlier"):          # x[0] of every channel k sigma of the rest away from it: 330 -> 314, 1000 -> 714 sigma of the whole channel
        k = float(kind[7:])
        x = x * 2.0 + 5.0
        x[:, 0] = 5.0 + k * 2.0 * torch.tensor([1.0, -1.0] * C)[:C]
    elif kind.startswith("spoil"):            # two of the kernels' three pivot samples far out on the same side: the median pivot IS an
        where, k = kind[6:9], float(kind[9:])  # outlier, and only the (n, mean, M2) merge keeps rstd (spoil_end: x[0], x[HW-1]; spoil_mid: x[0], x[HW/2])
        x = x * 2.0 + 5.0
        far = 5.0 + k * 2.0 * torch.tensor([1.0, -1.0] * C)[:C]
        x[:, 0] = far
        x[:, HW - 1 if where == "end" else HW // 2] = far
    return x.float()


NORM_CASES = [(3, 1, "plain"), (2, 3, "plain"), (1, 1000, "plain"), (5, 97 * 192, "plain"), (1, 97 * 192 + 1, "plain"),
              (2, 1000, "offset"), (2, 97 * 192, "offset"), (2, OUTLIER_HW, "outlier330"), (2, OUTLIER_HW + 3, "outlier330"),
              (2, OUTLIER_HW, "outlier1000"), (2, OUTLIER_HW, "spoil_end1000"), (2, OUTLIER_HW + 3, "spoil_end330"),
              (2, OUTLIER_HW, "spoil_mid330")]


def _pivot(x):
    """The pivot the kernels shift by (moments.h): the median of the first, middle and last element of each channel."""
    HW = x.shape[1]
    return x[:, [0, HW // 2, HW - 1]].double().median(1).values


def _norm_ref(x, g, b):
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return mean[:, 0], rstd[:, 0], (xd - mean) * rstd * g.double()[:, None] + b.double()[:, None]


@pytest.mark.parametrize("C,HW,kind", NORM_CASES, ids=[f"C{c}-HW{h}-{k}" for c, h, k in NORM_CASES])
def test_instance_stats_rstd_against_float64(C, HW, kind):
    """scale = gamma rstd within 1e-5; shift = beta - mean scale within 1e-5 of |beta| + |mean scale| (the fp32 mean of a field at 1e4
    is itself only good to ~6e-8 of 1e4), plus what the pivot costs the mean: a few roundings of |mean - pivot| (16 x 2^-24 of it), which
    matters only where the pivot is an outlier."""
    x = _norm_input(C, HW, kind, C * 7 + HW % 97)
    gen = torch.Generator().manual_seed(HW % 1000)
    g, b = 1 + 0.2 * torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    mean, rstd, _ = _norm_ref(x, g, b)
    CP = (C + 3) // 4 * 4 + 4
    tab = torch.full((2 * CP,), float("nan"), device=DEV)
    torch.ops.skyrim_hip.sfno_instance_stats(x.to(DEV), g.to(DEV), b.to(DEV), tab, CP, C, HW, EPS)
    t = tab.cpu().double()
    sc_ref = g.double() * rstd
    sh_ref = b.double() - mean * sc_ref
    err_rstd = ((t[:C] - sc_ref).abs() / sc_ref.abs()).max().item()
    print(f"instance_stats C={C} HW={HW} {kind}: rstd rel err {err_rstd:.3e}")
    assert err_rstd < 1e-5
    lim_sh = 1e-5 * (b.double().abs() + (mean * sc_ref).abs()) + 16 * 2.0 ** -24 * (mean - _pivot(x)).abs() * sc_ref.abs()
    err_sh = (t[CP:CP + C] - sh_ref).abs()
    print(f"instance_stats C={C} HW={HW} {kind}: shift err / bar {(err_sh / lim_sh).max().item():.3e}")
    assert (err_sh <= lim_sh).all()
    assert t[C:CP].isnan().all() and t[CP + C:].isnan().all()           # nothing beyond C channels is written


@pytest.mark.parametrize("C,HW,kind", NORM_CASES, ids=[f"C{c}-HW{h}-{k}" for c, h, k in NORM_CASES])
def test_instance_norm_against_float64(C, HW, kind):
    """Per channel: max|out - ref| <= 1e-5 max|ref| + 1e-6 |gamma| |mean| rstd -- the 1e-5 bar on rstd carried to the output, plus what
    the fp32 rounding of a large mean contributes (x g and the mean at 1e4 are good to ~6e-8 of 1e4 each); every element written (the
    output starts as NaN)."""
    x = _norm_input(C, HW, kind, C * 7 + HW % 97 + 1)
    gen = torch.Generator().manual_seed(HW % 1000 + 1)
    g, b = 1 + 0.2 * torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    mean, rstd, ref = _norm_ref(x, g, b)
    out = torch.full((C, HW), float("nan"), device=DEV)
    torch.ops.skyrim_hip.sfno_instance_norm(x.to(DEV), g.to(DEV), b.to(DEV), out, C, HW, EPS)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(1)
    lim = 1e-5 * ref.abs().amax(1) + 1e-6 * g.double().abs() * mean.abs() * rstd
    print(f"instance_norm C={C} HW={HW} {kind}: worst err / bar {(err / lim).max().item():.3e}")
    assert (err <= lim).all(), (err / lim)
