"""The float64 restatements of tests/_graphcast_reference.py, on the CPU: (1) composed into oracle.graphcast_oracle's mlp, edge_update
and aggregate on a small random graph they agree to 1e-12, so they are no private definition of the GraphCast building blocks; (2) the
bounds of tests/test_graphcast_kernels_gpu.py discriminate: a correct fp32 evaluation of each formula on the GPU test's own inputs stays
inside its bound, and each emulated kernel mistake -- a dropped lo plane of the weight or of the activation, a one-pass variance, a per-k
affine that stops one column short, an ignored K tail, a padding group summed into a real one, two swapped columns of a perm8 octet --
trips it."""
from __future__ import annotations

import pytest
import torch

import _graphcast_reference as R
from oracle import graphcast_oracle as O


# ---- the restatements against the oracle ------------------------------------------------------------------------------------------ #
def _mlp_params(name, k_in, L, g, ln=True):
    d = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    p = {f"{name}.fc1.weight": d(L, k_in) / k_in ** 0.5, f"{name}.fc1.bias": d(L), f"{name}.fc2.weight": d(L, L) / L ** 0.5, f"{name}.fc2.bias": d(L)}
    if ln:
        p[f"{name}.ln.weight"], p[f"{name}.ln.bias"] = 1 + 0.1 * d(L), 0.1 * d(L)
    return p


@pytest.fixture(scope="module")
def graph():
    """7 senders, 5 receivers with exactly three incoming edges each (so that the group-of-three sum applies), in random edge order."""
    g = R.gen(11)
    L, ns, nr = 16, 7, 5
    recv = torch.arange(nr).repeat_interleave(3)[torch.randperm(3 * nr, generator=g)]
    send = torch.randint(0, ns, (3 * nr,), generator=g)
    d = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    p = {**_mlp_params("edge", 3 * L, L, g), **_mlp_params("node", L, L, g)}
    return dict(L=L, ns=ns, nr=nr, edges=torch.stack([send, recv], 1), e=d(3 * nr, L), vs=d(ns, L), vr=d(nr, L), p=p)


def _close12(a, b):
    assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape
    assert ((a - b).abs().max() / b.abs().max()).item() < 1e-12


def test_mlp_is_gather_gemm_then_linear_layer_norm(graph):
    p, L, x = graph["p"], graph["L"], graph["vs"]
    want = O.mlp(p, "node", x)
    h = R.gather_gemm_ref([x], [None], [L], p["node.fc1.weight"], p["node.fc1.bias"], 2)
    _close12(R.linear_layer_norm_ref(h, L, p["node.fc2.weight"], p["node.fc2.bias"], p["node.ln.weight"], p["node.ln.bias"]), want)
    y = R.gather_gemm_ref([h], [None], [L], p["node.fc2.weight"], p["node.fc2.bias"], 0)
    _close12(R.layer_norm_ref(y, p["node.ln.weight"], p["node.ln.bias"]), want)
    res = graph["vs"] * 3
    _close12(R.layer_norm_ref(y, p["node.ln.weight"], p["node.ln.bias"], res), res + want)


def test_edge_update_both_ways(graph):
    """oracle.edge_update = gather_gemm over concat(e, v_s[send], v_r[recv]) + linear_layer_norm = sum_linear_layer_norm over the three terms."""
    p, L, ed = graph["p"], graph["L"], graph["edges"]
    e, vs, vr = graph["e"], graph["vs"], graph["vr"]
    want = O.edge_update(p, "edge", e, vs, vr, ed)
    w1, b1 = p["edge.fc1.weight"], p["edge.fc1.bias"]
    tail = (p["edge.fc2.weight"], p["edge.fc2.bias"], p["edge.ln.weight"], p["edge.ln.bias"])
    i_s, i_r = ed[:, 0].int(), ed[:, 1].int()
    h = R.gather_gemm_ref([e, vs, vr], [None, i_s, i_r], [L, L, L], w1, b1, 2)
    _close12(R.linear_layer_norm_ref(h, L, *tail), want)
    terms = [R.gather_gemm_ref([e], [None], [L], w1[:, :L], b1, 0), R.gather_gemm_ref([vs], [None], [L], w1[:, L:2 * L], None, 0),
             R.gather_gemm_ref([vr], [None], [L], w1[:, 2 * L:], None, 0)]
    for group in (0, 1):
        _close12(R.sum_linear_layer_norm_ref(terms, [None, i_s, i_r], L, 2, *tail, None, len(ed), group), want)
    _close12(R.sum_linear_layer_norm_ref(terms, [None, i_s, i_r], L, 2, *tail, e, len(ed)), e + want)


def test_aggregate_is_segment_sum_and_the_group_of_three(graph):
    p, L, ed, nr = graph["p"], graph["L"], graph["edges"], graph["nr"]
    y = O.edge_update(p, "edge", graph["e"], graph["vs"], graph["vr"], ed)
    want = O.aggregate(y, ed[:, 1], nr)
    order = torch.argsort(ed[:, 1], stable=True)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(ed[:, 1], minlength=nr).cumsum(0)]).int()
    acc0 = graph["e"][order]
    out, acc = R.segment_sum_ref(y[order], offsets, nr, acc0)
    _close12(out, want)
    _close12(acc, acc0 + y[order])
    assert R.segment_sum_ref(y[order], offsets, nr)[1] is None
    # an empty node and rows nobody owns
    o2, a2 = R.segment_sum_ref(y[order], torch.tensor([3, 3, 6]), 2, acc0)
    assert (o2[0] == 0).all() and torch.equal(a2[:3], acc0[:3]) and torch.equal(a2[6:], acc0[6:])
    _close12(o2[1], y[order][3:6].sum(0))
    # group == 3: the virtual row order over the receiver-sorted edges (member a of group g = edge 3 g + a)
    grp, mem = R.virtual_rows(nr)
    assert len(grp) == 48 and grp.max() == 15 and sorted(zip(grp.tolist(), mem.tolist())) == [(g_, a) for g_ in range(16) for a in range(3)]
    v = torch.arange(48)
    assert torch.equal(grp[v], 16 * (v // 48) + v % 16) and int(grp[16 + 2]) == 2 and int(mem[16 + 2]) == 1
    edge = torch.where(grp < nr, 3 * grp + mem, torch.zeros_like(grp))
    w1, b1 = p["edge.fc1.weight"], p["edge.fc1.bias"]
    es, ss, rs = graph["e"][order], ed[order, 0], ed[order, 1]
    terms = [es @ w1[:, :L].T + b1, graph["vs"] @ w1[:, L:2 * L].T, graph["vr"] @ w1[:, 2 * L:].T]
    got = R.sum_linear_layer_norm_ref(terms, [edge.int(), ss[edge].int(), rs[edge].int()], L, 2, p["edge.fc2.weight"], p["edge.fc2.bias"],
                                      p["edge.ln.weight"], p["edge.ln.bias"], None, nr, 3)
    _close12(got, want)


def test_assert_close_rejects_non_finite_values_and_shapes():
    ref = torch.ones(4, 4, dtype=torch.float64)
    assert R.assert_close(ref.float(), ref, 0.0, "same") == 0.0
    for bad in (float("nan"), float("inf")):
        got = ref.clone()
        got[1, 2] = bad
        with pytest.raises(AssertionError, match="non-finite"):
            R.assert_close(got, ref, 1e30, "x")
    with pytest.raises(AssertionError):
        R.assert_close(ref[:3], ref, 1.0, "shape")
    with pytest.raises(AssertionError, match="max"):
        R.assert_close(ref * (1 + 3e-6), ref, 2e-6, "x")
    R.assert_close(ref * (1 + 1e-6), ref, 2e-6, "x")


# ---- the bounds discriminate --------------------------------------------------------------------------------------------------------- #
def _trips(got, ref, bound, what):
    with pytest.raises(AssertionError):
        R.assert_close(got, ref, bound, what)


GATHER = [(129, 72), (300, 264), (1, 256)]


@pytest.mark.parametrize("M,N", GATHER)
@pytest.mark.parametrize("act", [0, 2])
def test_gather_gemm_bound_catches_a_dropped_lo_plane(M, N, act):
    c = R.shape_case(M, N)
    ref = R.gather_ref(c, act)
    R.assert_close(R.gather_fp32(c, act), ref, R.BAR3, "fp32")
    _trips(R.gather_fp32(c, act, w=R.split_hi(c["w"])), ref, R.BAR3, "(a) W rounded to fp16")
    _trips(R.gather_fp32(c, act, a_map=R.split_hi), ref, R.BAR3, "(b) A rounded to fp16")


@pytest.mark.parametrize("K,rows", [(8, 129), (40, 300), (512, 127), (520, 1)])
def test_linear_layer_norm_bound_catches_a_dropped_lo_plane(K, rows):
    c = R.linear_case(K, rows, seed=3000 + K + rows)
    ref = R.linear_layer_norm_ref(c["a"], K, c["w"], c["bias"], c["gamma"], c["beta"])
    R.assert_close(R.linear_fp32(c), ref, R.BAR_LN, "fp32")
    _trips(R.linear_fp32(c, w=R.split_hi(c["w"])), ref, R.BAR_LN, "(a) W rounded to fp16")
    _trips(R.linear_fp32(c, a_map=R.split_hi), ref, R.BAR_LN, "(b) A rounded to fp16")


@pytest.mark.parametrize("N", sorted(R.LN_OFFSET_FP32))
@pytest.mark.parametrize("with_res", [False, True])
def test_layer_norm_offset_bound_catches_the_one_pass_variance(N, with_res):
    """(c) on the offset rows of the GPU cases.  The recorded fp32 figure behind the bound is checked too: the two-pass formula in fp32
    on this machine is inside the bound (four times the figure) and no less than a quarter of the figure (its reduction order may differ
    from where the figure was recorded, so the two need not be equal)."""
    x, gamma, beta, res = R.ln_case("offset", 5, N, 100 + N)
    res = res if with_res else None
    ref = R.layer_norm_ref(x, gamma, beta, res)
    y = R.layer_norm_fp32(x, gamma, beta, res)
    err = R.assert_close(y, ref, R.ln_offset_bound(N, with_res), "two-pass fp32")
    assert err >= R.LN_OFFSET_FP32[N][with_res] / 4
    assert torch.equal(y[2], beta if res is None else res[2] + beta)          # the constant row
    _trips(R.layer_norm_fp32(x, gamma, beta, res, one_pass=True), ref, R.ln_offset_bound(N, with_res), "(c) one-pass variance")


@pytest.mark.parametrize("N", [8, 65, 1000])
def test_layer_norm_ordinary_bound_holds_in_fp32(N):
    x, gamma, beta, res = R.ln_case("ordinary", 5, N, 100 + N)
    R.assert_close(R.layer_norm_fp32(x, gamma, beta, res), R.layer_norm_ref(x, gamma, beta, res), R.BAR3, "fp32")


@pytest.mark.parametrize("widths", R.AFFINE_WIDTHS)
@pytest.mark.parametrize("act", [0, 2])
def test_gather_gemm_bound_catches_an_affine_that_stops_short(widths, act):
    """(d) sksfno_prepare_weight zero-fills the padding columns k >= K, so a shift applied there multiplies zeros and cannot show; the
    off-by-one in the other direction -- the last real column left without its scale and shift -- does."""
    c = R.affine_case(widths)
    assert c["kshift"].abs().max() > 10 and c["K"] % 32 != 0
    ref = R.gather_ref(c, act)
    R.assert_close(R.gather_fp32(c, act), ref, R.BAR3, "fp32")
    _trips(R.gather_fp32(c, act, affine_cols=c["K"] - 1), ref, R.BAR3, "(d) affine skips the last real column")


@pytest.mark.parametrize("act", [0, 2])
def test_gather_gemm_bound_catches_an_ignored_k_tail(act):
    c = R.gather_case((8, 8, 5), 129, 72, seed=2100, idx_kinds=(None, "rand", "rand"))
    ref = R.gather_ref(c, act)
    R.assert_close(R.gather_fp32(c, act), ref, R.BAR3, "fp32")
    _trips(R.gather_fp32(c, act, k_used=16), ref, R.BAR3, "(e) last K % 8 columns ignored")


@pytest.mark.parametrize("G,K", [(1, 40), (15, 8), (17, 40), (37, 512)])
def test_group_of_three_bound_catches_a_leaking_padding_group(G, K):
    c = R.group3_case(G, K, seed=4000 + G)
    ref = R.group3_ref(c)
    assert torch.isfinite(ref).all()
    R.assert_close(R.group3_fp32(c), ref, R.BAR_LN, "fp32")
    _trips(R.group3_fp32(c, leak=True), ref, R.BAR_LN, "(f) padding group summed into the last real group")


def test_identity_case_catches_swapped_columns_of_an_octet():
    c = R.identity_case(129, seed=5000)
    ref = R.linear_layer_norm_ref(c["a"], 512, c["w"], c["bias"], c["gamma"], c["beta"])
    R.assert_close(ref, R.layer_norm_ref(c["a"], c["gamma"], c["beta"]), 1e-15, "W = I")
    R.assert_close(R.linear_fp32(c), ref, R.BAR_LN, "fp32")
    assert len(set(c["gamma"].tolist())) == 512 and len(set(c["beta"].tolist())) == 512
    for i, j in ((0, 1), (259, 263), (504, 511)):                 # inside one octet of eight consecutive columns
        perm = torch.arange(512)
        perm[i], perm[j] = j, i
        _trips(R.linear_fp32(c, col_map=perm), ref, R.BAR_LN, f"(g) columns {i} and {j} swapped")


# ---- the fused kernels (tests/test_graphcast_fused_edges_gpu.py): the cases are well formed and the bounds bite ---------------------------- #
def test_run_structures_obey_the_header_and_hit_their_edges():
    """Every structure keeps the header's rule (a run crosses a tile boundary only if it is longer than a tile, its receivers are not
    met again later) within 12 tiles; the seams structure ends runs at rows 62, 63, 64, 126 and 127 of its first tile."""
    for name in R.RUN_STRUCTURES + ["mixed"]:
        recv, n_nodes = R.mixed_runs() if name == "mixed" else R.run_structure(name)
        assert len(recv) % R.TILE == 0 and len(recv) <= 12 * R.TILE and int(recv.max()) < n_nodes
        ends = [i for i in range(len(recv)) if recv[i] >= 0 and (i + 1 == len(recv) or recv[i + 1] != recv[i])]
        starts = [i for i in range(len(recv)) if recv[i] >= 0 and (i == 0 or recv[i - 1] != recv[i])]
        assert len({int(recv[i]) for i in starts}) == len(starts), name
        for i0, i1 in zip(starts, ends):
            assert i0 // R.TILE == i1 // R.TILE or i1 - i0 + 1 > R.TILE, (name, i0, i1)
        if name == "seams":
            assert [i for i in ends if i < R.TILE] == [62, 63, 64, 126, 127]
    lens = {int(n) for name in ("long_a", "long_b") for r in [R.run_structure(name)[0]] for n in torch.bincount(r[r >= 0])}
    assert {128, 129, 256, 257, 300, 389} <= lens
    assert R.continuations(R.run_structure("long_b")[0])[5] == [4, 5, 6]


@pytest.fixture(scope="module")
def sum_rows():
    """fp32 rows of the size of the edge kernel's y (LayerNorm output: unit scale, offset by beta), per structure."""
    def rows(name):
        recv, n_nodes = R.run_structure(name)
        y = (0.1 + torch.randn(len(recv), 64, generator=R.gen(9000 + len(recv)), dtype=torch.float64)).float()
        return recv, n_nodes, y
    return rows


@pytest.mark.parametrize("name", R.RUN_STRUCTURES)
@pytest.mark.parametrize("order", ["forward", "reverse", "pairwise"])
def test_summation_bound_accepts_fp32_sums_in_any_order(sum_rows, name, order):
    recv, n_nodes, y = sum_rows(name)
    got = R.fp32_run_sums(y, recv, n_nodes, order)
    ratio, excess = R.sum_bound_excess(got, y, recv, n_nodes)
    assert excess <= 0 and ratio <= 1
    has = torch.bincount(recv[recv >= 0], minlength=n_nodes) > 0
    assert torch.isnan(got[~has]).all()


@pytest.mark.parametrize("name,mistake", [("seams", "drop_last"), ("long_a", "drop_last"), ("singles", "drop_last"), ("long_a", "cont_to_next"), ("long_b", "cont_to_next"),
                                          ("mid", "cont_to_next"), ("seams", "miss_63")])
def test_summation_bound_rejects_the_mistakes_of_a_receiver_sum(sum_rows, name, mistake):
    recv, n_nodes, y = sum_rows(name)
    got = torch.nan_to_num(R.fp32_run_sums(y, recv, n_nodes, "forward", mistake))          # (a run that lost all its rows stays unwritten)
    ratio, excess = R.sum_bound_excess(got, y, recv, n_nodes)
    assert excess > 0 and ratio > 100, (ratio, excess)


@pytest.mark.parametrize("n_src,rows", [(1, 129), (2, 257), (2, 1)])
def test_node_bound_catches_a_dropped_lo_plane(n_src, rows):
    c = R.fused_node_case(n_src, rows, 8000 + 10 * rows + n_src)
    res = c["srcs"][0]
    ref = R.fused_node_ref(c, res)
    R.assert_close(R.fused_node_fp32(c, res), ref, R.BAR_LN, "fp32")
    _trips(R.fused_node_fp32(c, res, w2=R.split_hi(c["w2"])), ref, R.BAR_LN, "W2 rounded to fp16")
    _trips(R.fused_node_fp32(c, res, a_map=R.split_hi), ref, R.BAR_LN, "the operand rounded to fp16")


@pytest.mark.parametrize("n_src", [1, 2])
def test_node_offset_and_far_bounds_and_their_recorded_figures(n_src):
    """The recorded fp32 figures are reproduced (within a factor of 4 either way: the reduction order of this machine's fp32 products
    may differ from where they were recorded), and the offset-row bound rejects the one-pass variance."""
    c = R.fused_node_case(n_src, 129, 8100 + n_src, "offset")
    res = c["srcs"][0]
    ref = R.fused_node_ref(c, res)
    bound = R.LN_OFFSET_FACTOR * R.NODE_OFFSET_FP32[n_src]
    err = R.assert_close(R.fused_node_fp32(c, res), ref, bound, "two-pass fp32")
    assert err >= R.NODE_OFFSET_FP32[n_src] / 4
    _trips(R.fused_node_fp32(c, res, one_pass=True), ref, bound, "one-pass variance")
    c = R.fused_node_case(n_src, 129, 8200 + n_src, "far")
    far = list(R.FAR_ROWS)
    err = R.row_rel_err(R.fused_node_fp32(c, c["srcs"][0])[far], R.fused_node_ref(c, c["srcs"][0])[far])
    assert R.NODE_FAR_FP32[n_src] / 4 <= err <= R.LN_OFFSET_FACTOR * R.NODE_FAR_FP32[n_src]


def test_node_constant_rows_are_exact_in_fp32():
    c = R.fused_node_case(2, 5, 8502, "constant")
    assert torch.equal(R.fused_node_fp32(c), c["beta"].expand(5, 512))
    assert torch.equal(R.fused_node_fp32(c, c["srcs"][0]), c["srcs"][0] + c["beta"])


def test_edge_restatement_is_the_edge_mlp_by_distributivity():
    """fused_edge_ref is the edge MLP on concat(e, v_s[send], v_r[recv]) -- gather_gemm_ref + linear_layer_norm_ref, which
    test_mlp_is_gather_gemm_then_linear_layer_norm ties to oracle.graphcast_oracle -- up to the one rounding it adds to float64 operands,
    the fp16 plane of the hidden activation (2^-11 of each h): the restatement is no private definition."""
    recv, n_nodes = R.run_structure("seams")
    c = R.fused_edge_case(31, recv, n_nodes)
    g = R.gen(5)
    vs, vr = torch.randn(300, 512, generator=g, dtype=torch.float64), torch.randn(300, 512, generator=g, dtype=torch.float64)
    ws, wr = torch.randn(512, 512, generator=g, dtype=torch.float64) / 512 ** 0.5, torch.randn(512, 512, generator=g, dtype=torch.float64) / 512 ** 0.5
    b1 = 0.1 * torch.randn(512, generator=g, dtype=torch.float64)
    x = c["e"].double()
    a = torch.cat([x, vs[c["send"].long()], vr[c["near"].long()]], dim=1)
    w1 = torch.cat([c["w1"].double(), ws, wr], dim=1)
    want = R.linear_layer_norm_ref(R.gather_gemm_ref([a], [None], [1536], w1, b1, 2), 512, c["w2"], c["b2"], c["gamma"], c["beta"])
    c2 = dict(c, ts=vs @ ws.T + b1, tr=vr @ wr.T)
    got = R.fused_edge_ref(c2, 2, 2)
    # what is left: 512 roundings of 2^-11 / sqrt(3) of an h of unit size, through weights of variance 1 / 512 and a LayerNorm that divides
    # by a spread of about one half -- a mean |error| of a few 1e-4, on outputs whose maximum is about 5
    assert R.rel_err(got, want) < 1e-3 and (got - want).abs().mean() < 5e-4
