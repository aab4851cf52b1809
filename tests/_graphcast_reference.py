"""Float64 restatements of the GraphCast building blocks of include/skyrim_graphcast.h, written from the header's formulas with plain
torch on the CPU: one function per entry point (skgc_gather_gemm, skgc_layer_norm, skgc_segment_sum, skgc_linear_layer_norm,
skgc_sum_linear_layer_norm) and the virtual row order of skgc_sum_desc::group == 3; at the end of the file the fused kernels of ABI v4
(skgc_edge_update, skgc_segment_fixup, skgc_node_mlp) with their run structures and the bound of an fp32 sum, for
tests/test_graphcast_fused_edges_gpu.py.  They share nothing with the engine or the HIP side.  tests/test_graphcast_cpu.py composes them into oracle.graphcast_oracle's mlp / edge_update / aggregate (so they are no private
definition) and shows that the bounds of tests/test_graphcast_kernels_gpu.py separate a correct fp32 evaluation from the kernel
mistakes they are meant to catch; the inputs both files use are built here, from seeded generators, so that they are the same values.

Sources are 2-D tensors [n][ld] (a view that starts at the element offset of the call); only the first `width` columns are read."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

BAR3 = 2e-6                    # 3-term fp16 hi/lo products, fp32 accumulation: max|err| / max|ref| (tests/test_fuxi_kernels_gpu.py)
BAR_LN = 3e-6                  # Linear + LayerNorm: what tests/test_graphcast_gpu.py and test_node_mlp_vs_float64 assert
EPS = 1e-5


# ---- the header's formulas ------------------------------------------------------------------------------------------------------- #
def _rows(src, idx, M, width):
    s = src.double()[:, :width]
    return s[idx.long()[:M]] if idx is not None else s[:M]


def gather_gemm_ref(srcs, idxs, widths, w, bias, act, kscale=None, kshift=None, M=None):
    """out[m][n] = act(sum_k A(m, k) W[n][k] + bias[n]),  A(m, :) = concat_s src[s][idx[s] ? idx[s][m] : m][0 .. width[s]),
    A * kscale + kshift per k first; act 0 = none, 2 = swish.  M: rows (default: the length of the first index array / source)."""
    if M is None:
        M = len(idxs[0]) if idxs[0] is not None else srcs[0].shape[0]
    a = torch.cat([_rows(s, i, M, wd) for s, i, wd in zip(srcs, idxs, widths)], dim=1)
    if kscale is not None:
        a = a * kscale.double() + kshift.double()
    y = a @ w.double().T
    if bias is not None:
        y = y + bias.double()
    assert act in (0, 2)
    return F.silu(y) if act == 2 else y


def layer_norm_ref(x, gamma, beta, res=None, eps=EPS):
    """(res ? res : 0) + (x - mean) / sqrt(biased variance + eps) * gamma + beta over the last axis."""
    x = x.double()
    d = x - x.mean(-1, keepdim=True)
    y = d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * gamma.double() + beta.double()
    return y if res is None else res.double() + y


def segment_sum_ref(e, offsets, n_nodes, acc=None):
    """out[v] = sum of e[j], offsets[v] <= j < offsets[v + 1] (zeros for an empty run); acc[j] += e[j] on exactly those rows.
    Returns (out, acc); acc is None when none is given."""
    e = e.double()
    out = torch.zeros(n_nodes, e.shape[1], dtype=torch.float64)
    new = None if acc is None else acc.double().clone()
    for v in range(n_nodes):
        j0, j1 = int(offsets[v]), int(offsets[v + 1])
        out[v] = e[j0:j1].sum(0)
        if new is not None:
            new[j0:j1] += e[j0:j1]
    return out, new


def linear_layer_norm_ref(a, K, w, bias, gamma, beta, res=None):
    """(res ? res : 0) + LayerNorm(a[:, 0..K) W^T + bias) * gamma + beta."""
    y = a.double()[:, :K] @ w.double().T
    if bias is not None:
        y = y + bias.double()
    return layer_norm_ref(y, gamma, beta, res)


def virtual_rows(G):
    """(group, member) of every virtual input row of group == 3: row 48 t + 16 a + l is member a of group 16 t + l; 48 ceil(G / 16)
    rows, the groups >= G are padding."""
    v = torch.arange((G + 15) // 16 * 48)
    return 16 * (v // 48) + v % 16, (v % 48) // 16


def sum_linear_layer_norm_ref(srcs, idxs, K, act, w, bias, gamma, beta, res, rows, group=0):
    """(res ? res : 0) + LayerNorm(act(sum_s src[s][idx[s] ? idx[s][r] : r][0..K)) W^T + bias) * gamma + beta.  group 0 / 1: one output
    row per input row; group 3: `rows` groups, the index arrays are in virtual row order, out[g] = the sum over the three members."""
    assert act in (0, 2) and group in (0, 1, 3)
    M = rows if group != 3 else (rows + 15) // 16 * 48
    h = sum(_rows(s, i, M, K) for s, i in zip(srcs, idxs))
    if act == 2:
        h = F.silu(h)
    if group != 3:
        return linear_layer_norm_ref(h, K, w, bias, gamma, beta, res)
    assert res is None and all(i is not None for i in idxs)
    grp, _ = virtual_rows(rows)
    real = grp < rows
    y = linear_layer_norm_ref(h[real], K, w, bias, gamma, beta)
    return torch.zeros(rows, y.shape[1], dtype=torch.float64).index_add_(0, grp[real], y)


def rel_err(got, ref):
    """max|got - ref| / max|ref| in float64."""
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def assert_close(got, ref, bound, what):
    """max|got - ref| / max|ref| <= bound in float64; a non-finite value where the reference is finite fails.  Returns the error."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    bad = ~torch.isfinite(got) & torch.isfinite(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} non-finite values where the reference is finite"
    err = rel_err(got, ref)
    assert err <= bound, f"{what}: max|err| / max|ref| = {err:.3e} > {bound:.1e}"
    return err


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------------ #
def gen(seed):
    return torch.Generator().manual_seed(seed)


def weight(N, K, g):
    """fp32 [N][K] with random signs and magnitudes log-uniform over 1e-3 .. 10: no entry is an fp16 number, so the lo plane matters."""
    mag = 10.0 ** (4.0 * torch.rand(N, K, generator=g, dtype=torch.float64) - 3.0)
    w = (mag * (2.0 * torch.randint(0, 2, (N, K), generator=g) - 1.0)).float()
    w = torch.where(w.half().float() == w, w * (1.0 + 2.0 ** -13), w)          # one value in 2^13 is an fp16 number by chance
    assert (w.half().float() != w).all()
    return w


@functools.lru_cache(maxsize=None)
def weight_for(N, K):
    """THE weight of shape [N][K] of every case here: one matrix per shape, so that the GPU tests prepare each once."""
    return weight(N, K, gen(900000 + 1000 * N + K))


def vec(N, g, scale=1.0, offset=0.0):
    return (offset + scale * torch.randn(N, generator=g)).float()


def index(n, M, g, kind="rand"):
    """int32 [M] into n rows: random with the source's last row named at least once; `repeat`: one row for every m; `last`: n - 1."""
    if kind == "repeat":
        return torch.full((M,), n // 2, dtype=torch.int32)
    if kind == "last":
        return torch.full((M,), n - 1, dtype=torch.int32)
    i = torch.randint(0, n, (M,), generator=g).int()
    i[M // 2] = n - 1
    return i


def ln_rows(kind, rows, N, seed):
    """x [rows][N] of skgc_layer_norm's cases.  `ordinary`: unit normal.  `offset`: mean 1e4, spread 1, and row rows // 2 constant (1e4:
    every partial sum of up to 1024 of them is an fp32 integer, so the mean is exact and the row's output is exactly beta (+ res))."""
    g = gen(seed)
    x = torch.randn(rows, N, generator=g)
    if kind == "offset":
        x = (1e4 + x).float()
        x[rows // 2] = 1e4
    return x.float()


def ln_case(kind, rows, N, seed):
    """(x, gamma, beta, res) in fp32; gamma ~ 1."""
    x = ln_rows(kind, rows, N, seed)
    g = gen(seed + 1)
    return x, vec(N, g, 0.1, 1.0), vec(N, g, 0.5), torch.randn(rows, N, generator=g)


def layer_norm_fp32(x, gamma, beta, res=None, one_pass=False):
    """The kernel's two-pass formula in fp32 torch on the CPU (one_pass: variance as E[x^2] - mean^2 instead)."""
    x = x.float()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (x * x).mean(-1, keepdim=True) - mean * mean if one_pass else (d * d).mean(-1, keepdim=True)
    y = d * torch.rsqrt(var + torch.tensor(EPS)) * gamma + beta
    return y if res is None else res + y


# Offset rows of skgc_layer_norm: the bound is 4 x the error of layer_norm_fp32 (two-pass, fp32, torch on the CPU) against float64 on the
# same inputs, ln_case("offset", 5, N, 100 + N); the factor covers the device's reduction order and rsqrtf.  The error is that of the
# fp32 MEAN: near 1e4 it is rounded to 2^-10, a shift of up to 5e-4 of every x - mean against a spread of 1 (more for the few-sample
# rows of N = 8).  Measured max|err| / max|ref| per N, (without, with) the residual:
LN_OFFSET_FP32 = {
    8: (2.549e-04, 2.284e-04), 63: (3.262e-04, 2.701e-04), 64: (3.134e-04, 2.129e-04), 65: (1.547e-04, 1.556e-04),
    72: (1.720e-04, 1.198e-04), 512: (3.641e-04, 3.042e-04), 1000: (3.083e-04, 2.142e-04), 1024: (2.040e-04, 1.393e-04),
}
LN_OFFSET_FACTOR = 4.0


def ln_offset_bound(N, with_res):
    return LN_OFFSET_FACTOR * LN_OFFSET_FP32[N][1 if with_res else 0]


def split_hi(x):
    """What is left of fp32 values when the lo plane of the fp16 hi/lo split is dropped."""
    return x.half().float()


def gather_case(widths, M, N, seed, n_rows=(None, 40, 9), idx_kinds=(None, "rand", "rand"), affine=False, lds=None):
    """One skgc_gather_gemm case in fp32: sources [n][ld] (ld = lds[s] or the width), index arrays (None: rows m), W [N][K], bias, and
    with `affine` a per-k scale ~ 1 and a shift of order 10."""
    g = gen(seed)
    srcs, idxs = [], []
    for s, wd in enumerate(widths):
        kind = idx_kinds[s]
        n = M if kind is None else n_rows[s] or M + 3
        ld = wd if lds is None else lds[s]
        srcs.append(torch.randn(n, ld, generator=g))
        idxs.append(None if kind is None else index(n, M, g, kind))
    K = sum(widths)
    w, bias = weight_for(N, K), vec(N, g)
    ks, kh = (vec(K, g, 0.2, 1.0), vec(K, g, 10.0)) if affine else (None, None)
    return dict(srcs=srcs, idxs=idxs, widths=list(widths), w=w, bias=bias, kscale=ks, kshift=kh, M=M, N=N, K=K)


def gather_fp32(c, act, w=None, a_map=None, affine_cols=None, k_used=None):
    """skgc_gather_gemm's formula in fp32 torch, with hooks for the emulated mistakes: another weight, a map applied to the assembled A
    operand (after the affine), the affine on the first `affine_cols` columns only, only the first `k_used` columns of A read."""
    a = torch.cat([_rows(s, i, c["M"], wd).float() for s, i, wd in zip(c["srcs"], c["idxs"], c["widths"])], dim=1)
    if c["kscale"] is not None:
        n = c["K"] if affine_cols is None else affine_cols
        a = torch.cat([a[:, :n] * c["kscale"][:n] + c["kshift"][:n], a[:, n:]], dim=1)
    if k_used is not None:
        a = torch.cat([a[:, :k_used], torch.zeros(c["M"], c["K"] - k_used)], dim=1)
    if a_map is not None:
        a = a_map(a)
    y = a @ (c["w"] if w is None else w).T + c["bias"]
    return F.silu(y) if act == 2 else y


def gather_ref(c, act):
    return gather_gemm_ref(c["srcs"], c["idxs"], c["widths"], c["w"], c["bias"], act, c["kscale"], c["kshift"], c["M"])


def group3_case(G, K, seed, n_send=50):
    """The mesh->grid receiver sum: three edges into each of G nodes, in virtual row order.  Every source has one extra LAST row filled
    with 1e30, and the index entries of the padding groups (>= G) point at it: nothing of those rows may reach an output."""
    g = gen(seed)
    L = 512
    e, vs, vr = torch.randn(3 * G + 1, K, generator=g), torch.randn(n_send + 1, K, generator=g), torch.randn(G + 1, K, generator=g)
    for t in (e, vs, vr):
        t[-1] = 1e30
    send = torch.randint(0, n_send, (3 * G,), generator=g)
    grp, mem = virtual_rows(G)
    real = grp < G
    edge = torch.where(real, 3 * grp + mem, torch.full_like(grp, 3 * G))
    i_e = edge.int()
    i_s = torch.where(real, send[edge.clamp(max=3 * G - 1)], torch.full_like(grp, n_send)).int()
    i_r = torch.where(real, grp, torch.full_like(grp, G)).int()
    w, b2, gam, bet = weight_for(L, K), vec(L, g), vec(L, g, 0.1, 1.0), vec(L, g, 0.5)
    return dict(srcs=[e, vs, vr], idxs=[i_e, i_s, i_r], w=w, bias=b2, gamma=gam, beta=bet, G=G, K=K)


def identity_case(rows, seed):
    """W = I (K = 512) with gamma and beta distinct in every column: the output is LayerNorm(a) * gamma + beta, column for column."""
    g = gen(seed)
    L = 512
    a = torch.randn(rows, L, generator=g)
    gamma = (1.0 + torch.arange(L) / 256.0).float()[torch.randperm(L, generator=g)]
    beta = (torch.arange(L) / 64.0 - 4.0).float()[torch.randperm(L, generator=g)]
    return dict(a=a, w=torch.eye(L), bias=torch.zeros(L), gamma=gamma, beta=beta)


def shape_case(M, N):
    """The tile-edge cases of skgc_gather_gemm: widths (16, 8, 8); index arrays on none, some or all of the sources, by case."""
    kinds = [(None, None, None), (None, "rand", "rand"), ("rand", "rand", "rand")][(M + N) % 3]
    return gather_case((16, 8, 8), M, N, seed=1000 + 7 * M + N, idx_kinds=kinds)


AFFINE_WIDTHS = [(8, 8, 5), (32, 8)]           # K = 21 (a K tail inside the last 8-chunk) and K = 40 (a K tail of the 32-wide k-tile)


def affine_case(widths):
    return gather_case(widths, 129, 72, seed=2000 + sum(widths), idx_kinds=(None, "rand", "rand")[:len(widths)], affine=True)


def linear_case(K, rows, seed, lda_pad=4, bias50=False):
    """One skgc_linear_layer_norm case: a [rows][K + lda_pad] (row rows // 2 all zero when there are three or more), W [512][K], bias
    (bias50: 50 on every column, so the pre-norm rows are offset and the zero row gives exactly beta (+ res)), gamma ~ 1, beta, res."""
    g = gen(seed)
    L = 512
    a = torch.randn(rows, K + lda_pad, generator=g)
    if rows >= 3:
        a[rows // 2] = 0
    w = weight_for(L, K)
    bias = torch.full((L,), 50.0) if bias50 else vec(L, g)
    return dict(a=a, w=w, bias=bias, gamma=vec(L, g, 0.1, 1.0), beta=vec(L, g, 0.5), res=torch.randn(rows, L, generator=g), K=K, rows=rows)


def linear_fp32(c, w=None, a_map=None, col_map=None):
    """skgc_linear_layer_norm's formula in fp32 torch; hooks: another weight, a map of the A operand, a permutation of the pre-norm columns."""
    a = c["a"][:, :c["K"]] if "K" in c else c["a"]
    if a_map is not None:
        a = a_map(a)
    y = a @ (c["w"] if w is None else w).T + c["bias"]
    if col_map is not None:
        y = y[:, col_map]
    return layer_norm_fp32(y, c["gamma"], c["beta"])


def sum_case(n_src, idx_kinds, K, rows, seed, off=4, ld_pad=8):
    """One skgc_sum_linear_layer_norm case (group 0 / 1): sources [n][K + ld_pad] read from column `off` on, W [512][K], bias, gamma,
    beta, res.  views: what the reference reads."""
    g = gen(seed)
    L = 512
    bufs, idxs = [], []
    for s in range(n_src):
        kind = idx_kinds[s]
        n = rows if kind is None else (23, 9, 40)[s]
        bufs.append(torch.randn(n, K + ld_pad, generator=g))
        idxs.append(None if kind is None else index(n, rows, g, kind))
    return dict(bufs=bufs, views=[b[:, off:] for b in bufs], idxs=idxs, off=off, ld=K + ld_pad, K=K, rows=rows, w=weight_for(L, K), bias=vec(L, g),
                gamma=vec(L, g, 0.1, 1.0), beta=vec(L, g, 0.5), res=torch.randn(rows, L, generator=g))


def group3_fp32(c, leak=False):
    """group == 3 in fp32 torch; leak: the rows of the padding groups are summed into the last real group."""
    G, K = c["G"], c["K"]
    grp, _ = virtual_rows(G)
    h = F.silu(sum(s[i.long()][:, :K] for s, i in zip(c["srcs"], c["idxs"])))
    y = layer_norm_fp32(h @ c["w"].T + c["bias"], c["gamma"], c["beta"])
    keep = torch.ones_like(grp, dtype=torch.bool) if leak else grp < G
    return torch.zeros(G, 512).index_add_(0, grp[keep].clamp(max=G - 1), y[keep])


def group3_ref(c):
    return sum_linear_layer_norm_ref(c["srcs"], c["idxs"], c["K"], 2, c["w"], c["bias"], c["gamma"], c["beta"], None, c["G"], 3)


# ---- the fused kernels of ABI v4: skgc_edge_update, skgc_segment_fixup, skgc_node_mlp --------------------------------------------- #
# Restated from the header's formulas as the functions above are; nothing here imports the package.  The edge kernel rounds its edge
# operand, the hidden activation and (w1_planes == 1) W_e to ONE fp16 plane, and the restatement rounds in the same places (as
# tests/test_graphcast_fused_gpu.py does); the node kernel keeps fp16 hi/lo pairs and is held to BAR_LN like the other fp32-class kernels.
TILE = 128
U32 = 2.0 ** -24               # fp32 unit roundoff
BAR_AGG = 3e-4                 # receiver sums of the edge kernel, max|err| / max|ref|: what tests/test_graphcast_fused_gpu.py asserts
BAR_EOUT = 2e-3                # e_out, max|err| / max|ref| (one fp16 ulp where a rounding boundary is crossed), and its mean |err|:
BAR_EOUT_MEAN = 1e-4


def f16r(x):
    """The values of one fp16 plane, in float64."""
    return x.to(torch.float16).to(torch.float64)


def concat_runs(runs):
    """[(receiver, length), ...] -> the receiver of every packed row (int64), the runs laid down one after the other as given;
    receiver -1 = padding rows.  The caller places the tile boundaries: the total is a multiple of 128."""
    recv = torch.cat([torch.full((n,), r, dtype=torch.int64) for r, n in runs])
    assert len(recv) % TILE == 0
    return recv


def pack_runs(runs):
    """[(receiver, length), ...] packed by the header's rule: a run never crosses a 128-row tile unless it is longer than a tile (the
    tile is padded and the run starts the next one); the last tile is padded."""
    out, fill = [], 0
    for r, n in runs:
        if fill and n > TILE - fill:
            out.append((-1, TILE - fill))
            fill = 0
        out.append((r, n))
        fill = (fill + n) % TILE
    if fill:
        out.append((-1, TILE - fill))
    return concat_runs(out)


def run_structure(name):
    """(receiver of every packed row, n_nodes) of the receiver-sum cases.  one_run: a single-tile call that is one run, receiver 0.
    singles: 128 runs of one row, receiver 0 in row 0 and the highest node id in row 127.  seams: runs that end at rows 62, 63, 64, 126
    and 127 of a tile (the two 64-bit masks of run ends meet between rows 63 and 64), then two runs of 64, then 127 + 1.  long_a /
    long_b: runs of 128, 129, 256, 257 / 300, 3 * 128 + 5 rows, each followed by short runs, packed by the header's rule.  mid: a
    continuation piece that ends at row 39 of a tile, followed in that tile by the start of a run of 226 rows -- the header allows it
    (the run is longer than a tile), skyrim_amd.graphcast.fused.pack_segments never emits it.  pads: a tile that ends in padding, an
    all-padding tile in the middle and one at the end; no run continues, so the call needs no heads buffer."""
    if name == "one_run":
        return concat_runs([(0, 128)]), 3
    if name == "singles":
        return concat_runs([(2 * i, 1) for i in range(128)]), 255
    if name == "seams":
        return concat_runs([(0, 63), (1, 1), (3, 1), (4, 62), (7, 1), (8, 64), (9, 64), (10, 127), (12, 1)]), 13
    if name == "long_a":
        return pack_runs([(0, 128), (1, 3), (2, 1), (4, 40), (5, 129), (6, 2), (7, 17), (8, 256), (9, 1), (10, 30), (11, 257), (12, 5), (13, 1)]), 15
    if name == "long_b":
        return pack_runs([(0, 300), (2, 7), (3, 1), (5, 3 * 128 + 5), (6, 2), (7, 31)]), 9
    if name == "mid":
        return concat_runs([(1, 168), (4, 226), (5, 5), (6, 1), (-1, 112)]), 8
    if name == "pads":
        return concat_runs([(0, 5), (1, 40), (3, 20), (-1, 63), (-1, 128), (5, 1), (6, 100), (-1, 27), (-1, 128)]), 8
    raise KeyError(name)


RUN_STRUCTURES = ["one_run", "singles", "seams", "long_a", "long_b", "mid", "pads"]


def mixed_runs():
    """The run structure of the instantiation cases: short runs with a run of 300 and one of 130 among them (both continue over tiles)."""
    g = gen(77)
    short = torch.randint(1, 43, (25,), generator=g).tolist()
    lens = short[:15] + [300] + short[15:] + [1, 1, 130]
    return pack_runs([(2 * i, n) for i, n in enumerate(lens)]), 2 * len(lens) + 3


def continuations(recv):
    """{node: [tiles whose first run continues the node's run out of the previous tile]}, from the packed receivers."""
    out = {}
    for t in range(1, len(recv) // TILE):
        n = int(recv[t * TILE])
        if n >= 0 and int(recv[t * TILE - 1]) == n:
            out.setdefault(n, []).append(t)
    return out


def fused_edge_case(seed, recv, n_nodes, n_tab=300):
    """Operands of one skgc_edge_update case on the packed rows `recv`, with the statistics of tests/test_graphcast_fused_gpu.py: unit
    normal edge rows (held as the fp16 plane the kernel reads) and node-term tables, weights of variance 1 / 512, gamma ~ 1, b2 and beta
    of 0.1.  The node terms are gathered through `send` (random rows) and `near` (the row's receiver, as the processor does); padding rows
    have -1 in both and zeros in e."""
    g = gen(seed)
    L, rows = 512, len(recv)
    n_tab = max(n_tab, n_nodes)
    ok = recv >= 0
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    e = torch.where(ok[:, None], r(rows, L), torch.zeros(1, dtype=torch.float64)).half()
    send = torch.where(ok, torch.randint(0, n_tab, (rows,), generator=g), torch.full((rows,), -1))
    return dict(recv=recv.int(), ok=ok, n_nodes=n_nodes, rows=rows, e=e, send=send.int(), near=recv.int(),
                w1=(r(L, L) / L ** 0.5).float(), w2=(r(L, L) / L ** 0.5).float(), b2=(0.1 * r(L)).float(), gamma=(1 + 0.1 * r(L)).float(),
                beta=(0.1 * r(L)).float(), ts=r(n_tab, L).float(), tr=r(n_tab, L).float())


def fused_edge_ref(c, planes, n_term, w2=None, b2=None):
    """y [rows][512] in float64: LayerNorm(swish(pre) W2^T + b2) * gamma + beta with pre = (planes ? e W_e^T : e) + the first n_term of
    ts[send], tr[near]; planes 0 = the static form.  e is one fp16 plane, the hidden activation is rounded to one, W_e too when
    planes == 1.  (Padding rows gather row 0; nothing of them is used.)"""
    x = c["e"].double()
    pre = x if planes == 0 else x @ (c["w1"].double() if planes == 2 else f16r(c["w1"])).T
    for tab, ix in ((c["ts"], c["send"]), (c["tr"], c["near"]))[:n_term]:
        pre = pre + tab.double()[ix.long().clamp(min=0)]
    h = f16r(F.silu(pre))
    return layer_norm_ref(h @ (c["w2"] if w2 is None else w2).double().T + (c["b2"] if b2 is None else b2).double(), c["gamma"], c["beta"])


def run_sums(y, recv, n_nodes):
    """(sum, sum of |.|, rows) per receiver in float64; padding rows (recv < 0) belong to nobody."""
    ok = recv >= 0
    ix = recv[ok].long()
    s = torch.zeros(n_nodes, y.shape[1], dtype=torch.float64).index_add_(0, ix, y.double()[ok])
    m = torch.zeros(n_nodes, y.shape[1], dtype=torch.float64).index_add_(0, ix, y.double()[ok].abs())
    return s, m, torch.bincount(ix, minlength=n_nodes)


def sum_bound_excess(got, y, recv, n_nodes):
    """The receiver sums `got` [n_nodes][512] against the fp32 rows y they were taken over: an fp32 sum of len terms IN ANY ORDER is
    within len 2^-24 sum|y| of the exact sum, per column.  -> (the largest |error| / bound over the receivers that have rows, the
    largest |error| - bound); receivers without rows are not looked at.  A non-finite sum fails."""
    s, m, n = run_sums(y, recv, n_nodes)
    has = n > 0
    g = got.double()[has]
    assert torch.isfinite(g).all(), "a receiver sum is not finite"
    err, bound = (g - s[has]).abs(), n[has].double()[:, None] * U32 * m[has]
    return (err / bound.clamp_min(1e-300)).max().item(), (err - bound).max().item()


def fp32_run_sums(y, recv, n_nodes, order="forward", mistake=None):
    """The receiver sums taken in fp32 on the CPU, row by row: forward, reverse or pairwise inside a run.  mistake: `drop_last` leaves
    out every run's last row; `cont_to_next` adds the piece of a run that continues into a tile (the rows of that tile) to the NEXT
    receiver's sum; `miss_63` misses a run end at row 63 of a tile, so that run's rows are summed into the run that follows."""
    y = y.float()
    out = torch.full((n_nodes, y.shape[1]), float("nan"))
    recv = recv.tolist()
    starts = [i for i in range(len(recv)) if recv[i] >= 0 and (i == 0 or recv[i - 1] != recv[i])]
    carry = None

    def total(rows):
        if order == "pairwise":
            v = [y[i] for i in rows]
            while len(v) > 1:
                v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
            return v[0]
        acc = torch.zeros(y.shape[1])
        for i in (reversed(rows) if order == "reverse" else rows):
            acc = acc + y[i]
        return acc

    for k, i0 in enumerate(starts):
        i1 = i0
        while i1 < len(recv) and recv[i1] == recv[i0]:
            i1 += 1
        rows = list(range(i0, i1))
        moved = []
        if mistake == "drop_last":
            rows = rows[:-1]
        if mistake == "cont_to_next" and (i1 - 1) // TILE > i0 // TILE:
            cut = (i0 // TILE + 1) * TILE
            rows, moved = [i for i in rows if i < cut], [i for i in rows if i >= cut]
        s = total(rows) if rows else torch.zeros(y.shape[1])
        if carry is not None:
            s = s + carry
            carry = None
        if mistake == "miss_63" and (i1 - 1) % TILE == 63 and k + 1 < len(starts):
            carry = s
            continue
        if moved:
            carry = total(moved)
        out[recv[i0]] = s
    return out


def node_weight(N, K, g):
    """fp32 [N][K] of variance 1 / K (the statistics of tests/test_graphcast_fused_gpu.py) that holds no fp16 number, as `weight`."""
    w = (torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5).float()
    w = torch.where(w.half().float() == w, w * (1.0 + 2.0 ** -13), w)
    assert (w.half().float() != w).all()
    return w


@functools.lru_cache(maxsize=None)
def node_weights(n_src):
    """(W1 [512][512 n_src], W2 [512][512]) of every skgc_node_mlp case with n_src sources: prepared once by the GPU tests."""
    g = gen(910000 + n_src)
    return node_weight(512, 512 * n_src, g), node_weight(512, 512, g)


FAR_ROWS = (3, 64, 128)


def fused_node_case(n_src, rows, seed, kind="ordinary"):
    """One skgc_node_mlp case in fp32: sources of spread 3, b1, b2, beta of 0.1, gamma ~ 1, a residual buffer of its own.  kind
    `constant`: W2 = 0 and b2 = 4 on every column, so every pre-norm row is constant (the sum of 512 fours is exact in fp32) and the
    output is exactly beta (+ res).  `offset`: b2 = 1e4 + N(0, 1) on unit-scale products.  `far` (rows >= 129): rows FAR_ROWS of the
    sources are scaled so that the largest swish pre-activation of the row is 50 in size (before b1); both signs come out beyond 30."""
    g = gen(seed)
    L = 512
    srcs = [(3.0 * torch.randn(rows, L, generator=g, dtype=torch.float64)).float() for _ in range(n_src)]
    w1, w2 = node_weights(n_src)
    v = lambda s, o=0.0: (o + s * torch.randn(L, generator=g, dtype=torch.float64)).float()  # noqa: E731
    c = dict(srcs=srcs, w1=w1, w2=w2, b1=v(0.1), b2=v(0.1), gamma=v(0.1, 1.0), beta=v(0.1), res=torch.randn(rows, L, generator=g), rows=rows, n_src=n_src)
    if kind == "constant":
        c.update(w2=torch.zeros(L, L), b2=torch.full((L,), 4.0))
    elif kind == "offset":
        c["b2"] = v(1.0, 1e4)
    elif kind == "far":
        for r in FAR_ROWS:
            p = torch.cat([s[r] for s in srcs]).double() @ w1.double().T
            for s in srcs:
                s[r] *= 50.0 / p.abs().max().item()
    else:
        assert kind == "ordinary"
    return c


def node_pre_ref(c):
    """The swish pre-activations concat(src) W1^T + b1 in float64."""
    return torch.cat(c["srcs"], dim=1).double() @ c["w1"].double().T + c["b1"].double()


def fused_node_ref(c, res=None):
    """(res ? res : 0) + LayerNorm(swish(concat(src) W1^T + b1) W2^T + b2) * gamma + beta in float64."""
    return layer_norm_ref(F.silu(node_pre_ref(c)) @ c["w2"].double().T + c["b2"].double(), c["gamma"], c["beta"], res)


def fused_node_fp32(c, res=None, w2=None, a_map=None, one_pass=False):
    """The same formula in fp32 torch on the CPU (two-pass LayerNorm); hooks: another W2, a map of the concatenated operand, the
    one-pass variance."""
    a = torch.cat(c["srcs"], dim=1)
    if a_map is not None:
        a = a_map(a)
    h = F.silu(a @ c["w1"].T + c["b1"])
    return layer_norm_fp32(h @ (c["w2"] if w2 is None else w2).T + c["b2"], c["gamma"], c["beta"], res, one_pass)


def row_rel_err(got, ref):
    """max over the rows of max|got - ref| / max|ref| of the row, in float64."""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)).max().item()


# The node kernel's offset rows and far-out rows are handled as skgc_layer_norm's offset rows are: the bound is LN_OFFSET_FACTOR x the
# error of fused_node_fp32 against float64 on the same inputs (res = the first source).  NODE_OFFSET_FP32[n_src]: fused_node_case(n_src,
# 129, 8100 + n_src, "offset"), max|err| / max|ref| -- b2 near 1e4 puts every pre-norm value on a grid of 2^-10 against a spread of 1.4.
# NODE_FAR_FP32[n_src]: fused_node_case(n_src, 129, 8200 + n_src, "far"), rows FAR_ROWS, row_rel_err.
NODE_OFFSET_FP32 = {1: 8.902e-05, 2: 6.404e-05}
NODE_FAR_FP32 = {1: 6.006e-08, 2: 5.059e-08}
