"""The fused GraphCast kernels of include/skyrim_graphcast.h ABI v4 (csrc/graphcast_fused.hip: skgc_edge_update, skgc_segment_fixup,
skgc_node_mlp) at the edges the engine never reaches, against the float64 restatements of tests/_graphcast_reference.py and called the
way the engine calls them, torch.ops.skyrim_hip.gc_edge_update / gc_segment_fixup / gc_node_mlp (ctypes on the library only where the op
cannot express a case).  Conventions of tests/test_graphcast_kernels_gpu.py: every output starts as NaN with spare rows and a NaN margin
behind it, what a call does not own is still NaN afterwards, a refused call leaves all of it NaN, every measured error is printed next to
its bound (`ERR ...`).  The bounds are the project's own for these operands (R.BAR_AGG, R.BAR_EOUT, R.BAR_EOUT_MEAN, R.BAR_LN), the
derived bound of an fp32 sum in any order (R.sum_bound_excess), and R.LN_OFFSET_FACTOR x a recorded fp32-on-CPU figure;
tests/test_graphcast_cpu.py shows that each of them separates a correct evaluation from the mistakes it is meant to catch.

Which test launches which instantiation:
    edge_update_kernel<FC1, n_term, planes>
        <true, 0, 2> <true, 1, 2> <true, 2, 2>      test_edge_every_instantiation_vs_float64[2-*]
        <true, 0, 1> <true, 1, 1> <true, 2, 1>      test_edge_every_instantiation_vs_float64[1-*]
        <false, 0, 1> <false, 1, 1> <false, 2, 1>   test_edge_every_instantiation_vs_float64[0-*]      (<false, 1, 1>: the encoder's launch)
        <true, 2, 2> and <true, 2, 1> again         test_receiver_sum_by_run_structure (by structure), test_edge_constant_rows
    node_mlp_kernel<n_src>
        <1> <2>                                     test_node_rows_and_forms, test_node_constant_rows, test_node_offset_rows, test_node_far_out_swish
        <2>                                         test_node_strides_and_offsets, test_node_aliasing
    The refusals launch nothing."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import _graphcast_reference as R
from skyrim_amd.graphcast import fused as fz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 64                    # NaN elements past the end of every output
SPARE = 2                      # NaN rows past the rows a call owns
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


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    """Equal bit for bit, the NaN fill included."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _take(out, rows, N=L):
    """The rows a call owns, on the host; everything behind them must still be NaN."""
    torch.cuda.synchronize()
    o = out.cpu()
    assert _all_nan(o[rows * N:]), "a write past the rows of the call"
    return o[:rows * N].view(rows, N)


def _refused(call, *outs):
    with pytest.raises(RuntimeError, match=E_ARG):
        call()
    torch.cuda.synchronize()
    assert all(_all_nan(o) for o in outs), "a refused call wrote to an output"


# ---- skgc_edge_update + skgc_segment_fixup --------------------------------------------------------------------------------------------- #
class EdgeOperands:
    """The device side of an R.fused_edge_case: blocked fp16 edge rows (natural columns for the form with a first Linear, "pos" columns
    for the static form), the node-term tables in "pos" columns -- apart, and as the two halves of one [n_tab][1024] table -- and the
    weight fragments."""

    def __init__(self, c):
        self.c = c
        upos = torch.from_numpy(fz.unit_at_pos())
        e = c["e"].float()
        self.e_in = {True: fz.to_blocked_f16(e).to(DEV), False: fz.to_blocked_f16(e[:, upos]).to(DEV)}
        ts, tr = c["ts"][:, upos], c["tr"][:, upos]
        self.apart = [_d(ts), _d(tr)]
        self.table = _d(torch.cat([ts, tr], dim=1))
        self.idx = [_d(c["send"]), _d(c["near"])]
        w1 = c["w1"].to(DEV)
        self.w1f = {2: fz.prep_w1_fragments(w1, 2), 1: fz.prep_w1_fragments(w1, 1), 0: None}
        self.w2f = fz.prep_w2_fragments(c["w2"].to(DEV))
        self.tabs = [_d(c[k]) for k in ("b2", "gamma", "beta")]

    def blocked(self, e):
        return fz.to_blocked_f16(e.float()).to(DEV)


def run_edge(o, planes, n_term, recv, n_nodes, layout="table", e_in=None, e_out="new", heads=True, w2f=None, tabs=None):
    """One skgc_edge_update (+ skgc_segment_fixup where a run continues over tiles) on NaN-filled outputs.  planes 0 = the static form.
    e_out: "new" = a NaN-filled buffer of its own (with a first Linear only), None, or a tensor (e_in itself: in place).
    -> (agg [n_nodes][512] on the host, heads [tiles][512] on the host or None, e_out flat on the device or None)."""
    rows, fc1 = len(recv), planes > 0
    e_in = o.e_in[fc1] if e_in is None else e_in
    if isinstance(e_out, str):
        e_out = _nan(rows * L, torch.float16) if fc1 else None
    terms, offs, lds = ((o.apart, [0, 0], [L, L]) if layout == "apart" else ([o.table, o.table], [0, L], [2 * L, 2 * L]))
    agg = _nan((n_nodes + SPARE) * L)
    hd = _nan(rows // R.TILE * L) if heads else None
    recv_d = _d(recv.int())
    _hip().gc_edge_update(e_in, e_out, terms[:n_term], offs[:n_term], lds[:n_term], o.idx[:n_term], recv_d, o.w1f[planes], o.w2f if w2f is None else w2f,
                          *(o.tabs if tabs is None else tabs), agg, hd, rows, None, planes if fc1 else 2)
    nodes, first, tiles = fz.continuation_list(recv.numpy())
    want = R.continuations(recv)
    assert nodes.tolist() == sorted(want) and tiles.tolist() == [t for n in sorted(want) for t in want[n]] and first.tolist() == np.cumsum([0] + [len(want[n]) for n in sorted(want)]).tolist()
    if len(nodes):
        assert heads, "a run continues over tiles: the call needs a heads buffer"
        _hip().gc_segment_fixup(agg, hd, *(torch.from_numpy(a).to(DEV) for a in (nodes, first, tiles)))
    a = _take(agg, n_nodes)
    h = None
    if heads:
        h = _take(hd, rows // R.TILE)
        free = torch.ones(rows // R.TILE, dtype=torch.bool)
        free[tiles.astype(np.int64)] = False
        assert _all_nan(h[free]), "heads was written for a tile that continues no run"
        assert torch.isfinite(h[~free]).all()
    if e_out is not None and e_out is not e_in:
        assert _all_nan(e_out[rows * L:]), "a write past the rows of e_out"
    return a, h, e_out


def _rows16(flat, rows):
    """The packed rows [rows][512] of a blocked fp16 buffer, on the host."""
    return fz.from_blocked_f16(flat[:rows * L].cpu(), rows, L)


def _through_pack_segments(recv):
    """The packed receivers, rebuilt by the engine's packer from the receiver of every edge."""
    recv_e = recv[recv >= 0].numpy()
    row_edge = fz.pack_segments(recv_e)
    return torch.from_numpy(np.where(row_edge >= 0, recv_e[np.where(row_edge >= 0, row_edge, 0)], -1))


@pytest.fixture(scope="module")
def mixed():
    recv, n_nodes = R.mixed_runs()
    assert torch.equal(_through_pack_segments(recv), recv), "fused.pack_segments packs by another rule than the header's"
    assert len(recv) <= 12 * R.TILE and any(len(t) == 2 for t in R.continuations(recv).values())
    return EdgeOperands(R.fused_edge_case(31, recv, n_nodes))


INSTANCES = [(p, n, lay) for p in (2, 1, 0) for n, lays in ((0, ["none"]), (1, ["apart"]), (2, ["apart", "table"])) for lay in lays]


@pytest.mark.parametrize("planes,n_term,layout", INSTANCES, ids=[f"{p}-{n}-{lay}" for p, n, lay in INSTANCES])
def test_edge_every_instantiation_vs_float64(mixed, planes, n_term, layout):
    """The nine instantiations (first Linear with 2 or 1 weight planes, or the static form; 0, 1 or 2 gathered terms: each has its own
    count of gathers in flight and its own vmcnt immediates) on a run structure with a run of 300 and one of 130, with the fixup.  Terms
    with leading dimension 512 and offset 0, or both halves of one [n_tab][1024] table at offsets 0 and 512 (the processor's).  The
    `apart` case with two terms runs without e_out (the kernel's branch without the residual store)."""
    o, c = mixed, mixed.c
    recv, n_nodes, rows = c["recv"].long(), c["n_nodes"], c["rows"]
    y = R.fused_edge_ref(c, planes, n_term)
    ref, _, n = R.run_sums(y, recv, n_nodes)
    has = n > 0
    kw = dict(layout=layout, e_out=None if (layout == "apart" and n_term == 2) else "new")
    agg, heads, e_out = run_edge(o, planes, n_term, recv, n_nodes, **kw)
    assert _all_nan(agg[~has]), "a receiver without rows was written"
    assert torch.isfinite(agg[has]).all()
    err = ((agg[has].double() - ref[has]).abs().max() / ref.abs().max()).item()
    print(f"ERR edge_update planes={planes} n_term={n_term} {layout} receiver sums {err:.3e} / {R.BAR_AGG:.1e}")
    assert err < R.BAR_AGG
    if e_out is not None:
        out = _rows16(e_out, rows)
        assert _all_nan(out[~c["ok"]]), "a padding row of e_out was written"
        got, want = out[c["ok"]].double(), R.f16r(c["e"].double() + y)[c["ok"]]
        assert torch.isfinite(got).all()
        emax, emean = ((got - want).abs().max() / want.abs().max()).item(), (got - want).abs().mean().item()
        print(f"ERR edge_update planes={planes} n_term={n_term} {layout} e_out max {emax:.3e} / {R.BAR_EOUT:.1e} mean {emean:.3e} / {R.BAR_EOUT_MEAN:.1e}")
        assert emax < R.BAR_EOUT and emean < R.BAR_EOUT_MEAN
    agg2, heads2, e_out2 = run_edge(o, planes, n_term, recv, n_nodes, **kw)
    assert _same_bits(agg2, agg) and _same_bits(heads2, heads), "the second call gives other bits"
    assert e_out is None or _same_bits(e_out2, e_out)


def _f16_steps(a, b):
    """How many fp16 numbers apart two fp16 tensors are, element by element (0 = the same number; -0 = +0)."""
    key = lambda t: (lambda i: torch.where(i < 0, -(i & 0x7fff), i))(t.view(torch.int16).int())  # noqa: E731
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("name", R.RUN_STRUCTURES)
def test_receiver_sum_by_run_structure(name):
    """The receiver sum apart from the MFMA numerics.  Launch A gives every row a receiver of its own, so agg_A[r] is row r's fp32 y;
    launch B runs the structure under test on the same rows, and its sums are held to the bound of an fp32 sum of len terms in any
    order, len 2^-24 sum|y_A| per column -- a dropped or doubled row, a piece sent to the wrong receiver or a missed run end is orders
    above it.  Then: e_out = fp16(e_in + y_A) or its fp16 neighbour (the kernel's packed convert and the host's do not always agree next
    to a rounding boundary), padding rows of e_out untouched, the call in place gives the same bits, and the CONTENTS of padding rows are
    inert (6e4, then NaN, in their e_in)."""
    recv, n_nodes = R.run_structure(name)
    rows, tiles = len(recv), len(recv) // R.TILE
    assert tiles <= 12
    c = R.fused_edge_case(500 + R.RUN_STRUCTURES.index(name), recv, n_nodes)
    o, ok = EdgeOperands(c), c["ok"]
    planes = 2 - R.RUN_STRUCTURES.index(name) % 2
    cont = R.continuations(recv)
    if name in ("long_a", "long_b"):
        assert torch.equal(_through_pack_segments(recv), recv), "fused.pack_segments packs by another rule than the header's"
    if name == "long_b":
        assert max(len(t) for t in cont.values()) == 3, "one node has three head tiles"
    if name == "mid":
        assert cont == {1: [1], 4: [2, 3]} and int(recv[R.TILE + 39]) == 1 and int(recv[R.TILE + 40]) == 4
    if name == "pads":
        assert not cont and (recv[R.TILE:2 * R.TILE] < 0).all() and (recv[-R.TILE:] < 0).all() and recv[R.TILE - 1] < 0
    assert int(recv[0]) == 0 or name == "mid"                                  # receiver id 0 occurs

    y_a, _, _ = run_edge(o, planes, 2, torch.arange(rows), rows, heads=False)
    assert torch.isfinite(y_a[ok]).all()
    ref = R.fused_edge_ref(c, planes, 2)
    err = ((y_a[ok].double() - ref[ok]).abs().max() / ref[ok].abs().max()).item()
    print(f"ERR receiver_sum {name} planes={planes} rows of launch A {err:.3e} / {R.BAR_AGG:.1e}")
    assert err < R.BAR_AGG

    use_heads = name != "pads"                                                 # heads = None on a structure without continuations
    agg, heads, e_out = run_edge(o, planes, 2, recv, n_nodes, heads=use_heads)
    has = torch.bincount(recv[recv >= 0], minlength=n_nodes) > 0
    assert _all_nan(agg[~has]), "a receiver without rows was written"
    ratio, excess = R.sum_bound_excess(agg, y_a, recv, n_nodes)
    print(f"ERR receiver_sum {name} planes={planes} error / bound {ratio:.3e} / 1")
    assert excess <= 0
    out = _rows16(e_out, rows)
    assert _all_nan(out[~ok]), "a padding row of e_out was written"
    want = (c["e"].float() + y_a).half()
    steps = _f16_steps(out[ok], want[ok])
    print(f"ERR receiver_sum {name} e_out: {int((steps == 1).sum())} of {steps.numel()} are the fp16 neighbour, largest distance {int(steps.max())} / 1")
    assert torch.isfinite(out[ok]).all() and int(steps.max()) <= 1

    alias = o.e_in[True].clone()
    agg2, heads2, _ = run_edge(o, planes, 2, recv, n_nodes, heads=use_heads, e_in=alias, e_out=alias)
    torch.cuda.synchronize()
    assert _same_bits(agg2, agg) and (heads is None or _same_bits(heads2, heads)), "in place: other receiver sums"
    inplace = _rows16(alias, rows)
    assert _same_bits(inplace[ok], out[ok]) and not inplace[~ok].any(), "in place: other edge rows, or a padding row written"

    for fill in (6e4, float("nan")):
        e = c["e"].clone()
        e[~ok] = fill
        agg3, heads3, e_out3 = run_edge(o, planes, 2, recv, n_nodes, heads=use_heads, e_in=o.blocked(e))
        out3 = _rows16(e_out3, rows)
        assert _same_bits(agg3, agg) and (heads is None or _same_bits(heads3, heads)), f"padding rows of {fill} reach the sums"
        assert _same_bits(out3[ok], out[ok]) and _all_nan(out3[~ok]), f"padding rows of {fill} reach e_out"


def test_edge_constant_rows():
    """W2 = 0 and b2 = 4: every pre-norm row is constant and its mean is exact, so y is exactly beta on every row; the sums over the
    runs are inside the summation bound.  Without e_out."""
    recv, n_nodes = R.run_structure("seams")
    rows = len(recv)
    c = R.fused_edge_case(600, recv, n_nodes)
    o = EdgeOperands(c)
    w2f = fz.prep_w2_fragments(torch.zeros(L, L, device=DEV))
    tabs = [torch.full((L,), 4.0, device=DEV)] + o.tabs[1:]
    y_a, _, _ = run_edge(o, 2, 2, torch.arange(rows), rows, heads=False, e_out=None, w2f=w2f, tabs=tabs)
    assert torch.equal(y_a, c["beta"].expand(rows, L)), "a constant row gives exactly beta"
    agg, _, _ = run_edge(o, 2, 2, recv, n_nodes, e_out=None, w2f=w2f, tabs=tabs)
    ratio, excess = R.sum_bound_excess(agg, y_a, recv, n_nodes)
    print(f"ERR edge_update constant rows error / bound {ratio:.3e} / 1")
    assert excess <= 0


# ---- skgc_node_mlp ------------------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def node_w():
    """The weight fragments of R.node_weights(n_src), prepared once."""
    cache = {}

    def get(n_src):
        if n_src not in cache:
            w1, w2 = R.node_weights(n_src)
            cache[n_src] = (fz.prep_w1_node(w1.to(DEV)), fz.prep_w2_fragments(w2.to(DEV)))
        return cache[n_src]

    return get


def call_node(c, W, srcs, res, out, rows, w2f=None):
    """srcs / res / out: (tensor, element offset, leading dimension); res may be None."""
    _hip().gc_node_mlp([t for t, _, _ in srcs], [f for _, f, _ in srcs], [d for _, _, d in srcs], W[0], W[1] if w2f is None else w2f,
                       *(_d(c[k]) for k in ("b1", "b2", "gamma", "beta")), *(res if res is not None else (None, 0, L)), *out, rows)


def run_node(c, W, with_res=True, w2f=None):
    """The plain form: dense sources, the residual = the first source (as the engine's node updates), a NaN-filled output of its own."""
    rows = c["rows"]
    sd = [(_d(s), 0, L) for s in c["srcs"]]
    out = _nan((rows + SPARE) * L)
    call_node(c, W, sd, sd[0] if with_res else None, (out, 0, L), rows, w2f)
    return _take(out, rows)


@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 257])
def test_node_rows_and_forms(node_w, rows, n_src):
    c = R.fused_node_case(n_src, rows, 8000 + 10 * rows + n_src)
    err = R.assert_close(run_node(c, node_w(n_src)), R.fused_node_ref(c, c["srcs"][0]), R.BAR_LN, f"node_mlp rows={rows} n_src={n_src}")
    print(f"ERR node_mlp rows={rows} n_src={n_src} {err:.3e} / {R.BAR_LN:.1e}")


def test_node_strides_and_offsets(node_w):
    """Both sources and the residual out of one [rows][1536] buffer (column offsets 0, 1024 and 512), the output at column 64 of rows of
    640: the columns outside the 512 written and the rows past `rows` stay NaN."""
    rows, ldo = 129, 640
    c = R.fused_node_case(2, rows, 8300)
    buf = _d(torch.cat([c["srcs"][0], c["res"], c["srcs"][1]], dim=1)).flatten()
    out = _nan((rows + SPARE) * ldo)
    call_node(c, node_w(2), [(buf, 0, 3 * L), (buf, 2 * L, 3 * L)], (buf, L, 3 * L), (out, 64, ldo), rows)
    o = _take(out, rows + SPARE, ldo)
    mine = torch.zeros(rows + SPARE, ldo, dtype=torch.bool)
    mine[:rows, 64:64 + L] = True
    assert _all_nan(o[~mine]), "a write outside the 512 columns of the rows of the call"
    err = R.assert_close(o[mine].view(rows, L), R.fused_node_ref(c, c["res"]), R.BAR_LN, "node_mlp strides")
    print(f"ERR node_mlp ld 1536 / ld_out 640 {err:.3e} / {R.BAR_LN:.1e}")


@pytest.mark.parametrize("mode", ["res-absent", "res=src1", "out=src1", "out=res"])
def test_node_aliasing(node_w, mode):
    """Two sources with every aliasing the header allows: the bits of the same call with every buffer apart, and float64."""
    rows = 129
    c = R.fused_node_case(2, rows, 8400)
    W = node_w(2)
    s0, s1 = ((_d(s), 0, L) for s in c["srcs"])
    res_h = {"res-absent": None, "res=src1": c["srcs"][1], "out=src1": c["srcs"][0], "out=res": c["res"]}[mode]
    plain = _nan((rows + SPARE) * L)
    call_node(c, W, [s0, s1], None if res_h is None else (_d(res_h.clone()), 0, L), (plain, 0, L), rows)
    want = _take(plain, rows)
    err = R.assert_close(want, R.fused_node_ref(c, res_h), R.BAR_LN, f"node_mlp {mode}")
    print(f"ERR node_mlp {mode} {err:.3e} / {R.BAR_LN:.1e}")
    if mode == "res-absent":
        return
    buf = _nan((rows + SPARE) * L)                                   # the buffer that is written: a copy of the aliased operand in its first rows
    if mode == "res=src1":
        call_node(c, W, [s0, s1], s1, (buf, 0, L), rows)
    elif mode == "out=src1":
        buf[:rows * L] = s1[0].flatten()
        call_node(c, W, [s0, (buf, 0, L)], s0, (buf, 0, L), rows)
    else:
        buf[:rows * L] = _d(c["res"]).flatten()
        call_node(c, W, [s0, s1], (buf, 0, L), (buf, 0, L), rows)
    assert _same_bits(_take(buf, rows), want), f"{mode}: other bits than with every buffer apart"


@pytest.mark.parametrize("n_src", [1, 2])
def test_node_constant_rows(node_w, n_src):
    """W2 = 0 and b2 = 4: every pre-norm row is constant with an exact mean, and the output is exactly beta (+ res)."""
    c = R.fused_node_case(n_src, 129, 8500 + n_src, "constant")
    w2f = fz.prep_w2_fragments(torch.zeros(L, L, device=DEV))
    assert torch.equal(run_node(c, node_w(n_src), with_res=False, w2f=w2f), c["beta"].expand(129, L))
    assert torch.equal(run_node(c, node_w(n_src), w2f=w2f), c["srcs"][0] + c["beta"])


@pytest.mark.parametrize("n_src", [1, 2])
def test_node_offset_rows(node_w, n_src):
    """b2 = 1e4 + N(0, 1) on unit-scale products: handled as skgc_layer_norm's offset rows, LN_OFFSET_FACTOR x the error of the same
    two-pass formula in fp32 on the CPU (R.NODE_OFFSET_FP32)."""
    c = R.fused_node_case(n_src, 129, 8100 + n_src, "offset")
    bound = R.LN_OFFSET_FACTOR * R.NODE_OFFSET_FP32[n_src]
    err = R.assert_close(run_node(c, node_w(n_src)), R.fused_node_ref(c, c["srcs"][0]), bound, f"node_mlp offset rows n_src={n_src}")
    print(f"ERR node_mlp offset n_src={n_src} {err:.3e} / {bound:.3e} (fp32 on the CPU: {R.NODE_OFFSET_FP32[n_src]:.3e})")


@pytest.mark.parametrize("n_src", [1, 2])
def test_node_far_out_swish(node_w, n_src):
    """Swish pre-activations out to +50 and -50 in rows R.FAR_ROWS (checked on the float64 pre-activations): finite everywhere, the
    other rows inside R.BAR_LN, the far rows -- relative to the row's own maximum -- inside LN_OFFSET_FACTOR x the fp32-on-CPU figure."""
    c = R.fused_node_case(n_src, 129, 8200 + n_src, "far")
    far = list(R.FAR_ROWS)
    rest = [r for r in range(129) if r not in far]
    pre = R.node_pre_ref(c)
    top = pre[far].abs().amax(1)
    assert (top > 49).all() and (top < 51).all() and pre[far].max() > 30 and pre[far].min() < -30 and pre[rest].abs().max() < 25
    got, ref = run_node(c, node_w(n_src)), R.fused_node_ref(c, c["srcs"][0])
    assert torch.isfinite(got).all()
    err = R.assert_close(got[rest], ref[rest], R.BAR_LN, f"node_mlp far n_src={n_src}, the other rows")
    print(f"ERR node_mlp far n_src={n_src} other rows {err:.3e} / {R.BAR_LN:.1e}")
    bound = R.LN_OFFSET_FACTOR * R.NODE_FAR_FP32[n_src]
    rel = R.row_rel_err(got[far], ref[far])
    print(f"ERR node_mlp far n_src={n_src} far rows, relative to the row {rel:.3e} / {bound:.3e} (fp32 on the CPU: {R.NODE_FAR_FP32[n_src]:.3e})")
    assert rel <= bound


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------- #
def test_edge_update_refusals():
    from skyrim_amd.graphcast.engine import EdgeDesc
    recv, n_nodes = R.run_structure("seams")
    rows = len(recv)
    o = EdgeOperands(R.fused_edge_case(700, recv, n_nodes))
    agg, heads, e_out = _nan((n_nodes + SPARE) * L), _nan(rows // R.TILE * L), _nan(rows * L, torch.float16)
    recv_d = _d(recv.int())

    def call(rows=rows, ld=2 * L, e_in=o.e_in[True], e_out=e_out, w1f=o.w1f[2], planes=2):
        return lambda: _hip().gc_edge_update(e_in, e_out, [o.table, o.table], [0, L], [2 * L, ld], o.idx, recv_d, w1f, o.w2f, *o.tabs, agg, heads, rows, None, planes)

    outs = (agg, heads, e_out)
    _refused(call(rows=130), *outs)                                            # no multiple of 128
    _refused(call(rows=0), *outs)
    _refused(call(ld=508), *outs)                                              # ld < 512
    _refused(call(ld=514), *outs)                                              # ld % 4 != 0
    shifted = torch.cat([o.e_in[True], torch.zeros(8, dtype=torch.float16, device=DEV)])[4:]
    assert shifted.data_ptr() % 16 == 8
    _refused(call(e_in=shifted), *outs)                                        # e_in off by 8 bytes
    _refused(call(e_in=o.e_in[False], w1f=None), *outs)                        # e_out given to the static form
    _refused(call(w1f=torch.cat([o.w1f[2], o.w1f[1]]), planes=3), *outs)       # w1_planes == 3
    # n_term == 3: the op refuses it itself, so this goes to the library
    d = EdgeDesc()
    d.e_in, d.e_out = o.e_in[True].data_ptr(), e_out.data_ptr()
    for s in range(2):
        d.term[s], d.idx[s], d.ld[s] = o.table.data_ptr() + 4 * L * s, o.idx[s].data_ptr(), 2 * L
    d.recv, d.w1f, d.w2f = recv_d.data_ptr(), o.w1f[2].data_ptr(), o.w2f.data_ptr()
    d.b2, d.gamma, d.beta = (t.data_ptr() for t in o.tabs)
    d.agg, d.heads, d.rows, d.has_fc1, d.w1_planes = agg.data_ptr(), heads.data_ptr(), rows, 1, 2
    for n_term in (3, -1):
        d.n_term = n_term
        assert _lib().skgc_edge_update(ctypes.byref(d), _stream()) == -1
    torch.cuda.synchronize()
    assert all(_all_nan(t) for t in outs)


def test_node_mlp_refusals(node_w):
    from skyrim_amd.graphcast.engine import NodeDesc
    rows = 5
    c = R.fused_node_case(2, rows + 1, 8600)                                   # one row more than the call takes: room for a shifted source
    W = node_w(2)
    s0, s1 = (_d(s).flatten() for s in c["srcs"])
    out = _nan((rows + SPARE) * L)

    def call(rows=rows, off0=0, ld_res=L, ld_out=L):
        return lambda: call_node(c, W, [(s0, off0, L), (s1, 0, L)], (s0, 0, ld_res), (out, 0, ld_out), rows)

    _refused(call(rows=0), out)
    _refused(call(ld_out=508), out)
    _refused(call(ld_res=514), out)
    _refused(call(off0=1), out)                                                # a source off by 4 bytes
    # n_src of 0 and of 3: the op refuses them itself
    keep = [_d(c[k]) for k in ("b1", "b2", "gamma", "beta")]
    d = NodeDesc()
    d.src[0], d.src[1], d.ld[0], d.ld[1] = s0.data_ptr(), s1.data_ptr(), L, L
    d.w1f, d.w2f = W[0].data_ptr(), W[1].data_ptr()
    d.b1, d.b2, d.gamma, d.beta = (t.data_ptr() for t in keep)
    d.res, d.ld_res, d.out, d.ld_out, d.rows = None, L, out.data_ptr(), L, rows
    for n_src in (0, 3):
        d.n_src = n_src
        assert _lib().skgc_node_mlp(ctypes.byref(d), _stream()) == -1
    torch.cuda.synchronize()
    assert _all_nan(out)


def test_segment_fixup_refusals():
    agg, heads = _nan(4 * L), _nan(2 * L)
    none, one = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    _hip().gc_segment_fixup(agg, heads, none, one, none)                       # n_nodes == 0: nothing to do
    two = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    assert _lib().skgc_segment_fixup(agg.data_ptr(), heads.data_ptr(), one.data_ptr(), two.data_ptr(), one.data_ptr(), -1, _stream()) == -1
    torch.cuda.synchronize()
    assert _all_nan(agg) and _all_nan(heads)
