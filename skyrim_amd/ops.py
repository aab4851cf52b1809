"""``torch.ops.skyrim_hip.*`` -- the Python-side call path into the HIP kernels ("wrapped as torch.library custom ops").

Every op is a thin dispatcher entry over one ``extern "C"`` launcher of include/skyrim_{pangu,sfno,graphcast}.h: the op validates
its tensors (device, dtype, contiguity), takes the device guard and torch's CURRENT stream of that device, and calls the C ABI with
raw pointers.  Only the CUDA (= ROCm) dispatch key is registered: calling an op with CPU tensors raises NotImplementedError from the
dispatcher -- there is no CPU fallback.  Outputs are written in place into caller-owned tensors (schema ``Tensor(a!)``), so the ops
are stream-ordered, allocation-free and capturable in a HIP graph.

    pangu_step / pangu_patch_embed / pangu_block / pangu_downsample / pangu_upsample / pangu_patch_recover     (ctx = skpangu_ctx*)
    sfno_gemm / sfno_instance_norm / sfno_chain / sfno_instance_stats
    gc_gather_gemm / gc_linear_layer_norm / gc_sum_linear_layer_norm / gc_layer_norm / gc_segment_sum
    gc_edge_update / gc_segment_fixup / gc_node_mlp      (the fused interaction-network updates, csrc/graphcast_fused.hip)
    fcn_layer_norm / fcn_mlp / fcn_spectral_mlp          (FourCastNet v1, include/skyrim_fcn.h)
    dlwp_ingest / dlwp_conv / dlwp_egress                (DLWP, include/skyrim_dlwp.h)
    fuxi_layer_norm / fuxi_window_attention / fuxi_resample   (FuXi, include/skyrim_fuxi.h)
    fengwu_layer_norm / fengwu_window_attention             (FengWu, include/skyrim_fengwu.h)
    ens_perturb / ens_stats                              (ensemble members and statistics, include/skyrim_ens.h)
    score_fields                                         (forecast scores against a truth state, include/skyrim_score.h)
    noise_coeffs / noise_apply                           (spherical perturbations, include/skyrim_noise.h)
    track_detect                                         (cyclone candidates of M states, include/skyrim_track.h)
    derive_fields                                        (derived channels of M states, include/skyrim_derive.h)
    thermo_fields                                        (column thermodynamics of M states, include/skyrim_thermo.h)
    vert_fields                                          (fields of M states on chosen surfaces, include/skyrim_vert.h)
    regrid                                               (M states on another lat-lon grid, include/skyrim_regrid.h)
    event_counts                                         (joint counts and neighbourhood sums of threshold events, include/skyrim_event.h)
    agg_update                                           (one lead time folded into the time-window aggregates, include/skyrim_agg.h)
    nbr_fields                                           (max, min, mean, fraction above over great-circle discs, include/skyrim_nbr.h)
    point_gather                                         (M states sampled at scattered points, include/skyrim_point.h)
    gram / member_combine                                (member Gram matrices and linear combinations of M states, include/skyrim_gram.h)
    zonal_spectra                                        (zonal power spectra of M states, their mean, spread and errors, include/skyrim_spec.h)
    breed_norms / breed_apply                            (the two passes of a breeding cycle over M states, include/skyrim_breed.h)
    stoch_coeffs / stoch_evolve / stoch_apply            (per-step stochastic perturbations: SPPT and additive, include/skyrim_stoch.h)
    object_label / object_attributes / object_probability    (labelled threshold regions of M states, include/skyrim_object.h)
    clim_extremes / clim_quantiles                       (EFI, SOT and tail odds of M states against a quantile climate; the climate from N samples, include/skyrim_clim.h)
    pack_range / pack_quantize / pack_unpack             (M states as 16-bit big-endian codes with a per-plane table, and the way back, include/skyrim_pack.h)
"""
from __future__ import annotations

import ctypes

import torch

from . import native

_NS = "skyrim_hip"
_lib = torch.library.Library(_NS, "DEF")
_registered = False


def _f32(t: torch.Tensor, what: str, dev=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or (dev is not None and t.device != dev):
        raise ValueError(f"{what}: expected a contiguous float32 tensor on {dev or 'the GPU'}")
    return ctypes.c_void_p(t.data_ptr())


def _i32(t, what: str, dev):
    if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous int32 tensor on {dev}")
    return t.data_ptr()


def _f16(t, what: str, dev):
    if t.dtype != torch.float16 or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float16 tensor on {dev}")
    return t.data_ptr()


def _opt(t, off_bytes: int = 0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off_bytes)


# ---- Pangu ---------------------------------------------------------------------------------------------------------------- #
def _pangu():
    from .pangu import engine
    return engine.load_library()


def _pangu_step(ctx: int, x: torch.Tensor, out: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(x.device):
        native.check(lib.skpangu_step(ctypes.c_void_p(ctx), _f32(x, "x"), _f32(out, "out", x.device), native.stream(x.device)), "skpangu_step", lib)


def _pangu_patch_embed(ctx: int, x: torch.Tensor, out: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(x.device):
        native.check(lib.skpangu_patch_embed(ctypes.c_void_p(ctx), _f32(x, "x"), _f32(out, "out", x.device), native.stream(x.device)), "skpangu_patch_embed", lib)


def _pangu_block(ctx: int, layer: int, block: int, x: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(x.device):
        native.check(lib.skpangu_block(ctypes.c_void_p(ctx), layer, block, _f32(x, "x"), native.stream(x.device)), "skpangu_block", lib)


def _pangu_downsample(ctx: int, x1: torch.Tensor, out: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(x1.device):
        native.check(lib.skpangu_downsample(ctypes.c_void_p(ctx), _f32(x1, "x1"), _f32(out, "out", x1.device), native.stream(x1.device)), "skpangu_downsample", lib)


def _pangu_upsample(ctx: int, x2: torch.Tensor, out: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(x2.device):
        native.check(lib.skpangu_upsample(ctypes.c_void_p(ctx), _f32(x2, "x2"), _f32(out, "out", x2.device), native.stream(x2.device)), "skpangu_upsample", lib)


def _pangu_patch_recover(ctx: int, skip: torch.Tensor, x4: torch.Tensor, out: torch.Tensor) -> None:
    lib = _pangu()
    with torch.cuda.device(skip.device):
        native.check(lib.skpangu_patch_recover(ctypes.c_void_p(ctx), _f32(skip, "skip"), _f32(x4, "x4", skip.device), _f32(out, "out", skip.device), native.stream(skip.device)),
            "skpangu_patch_recover", lib)


# ---- SFNO ------------------------------------------------------------------------------------------------------------------ #
# geometry vector of sfno_gemm, in this order
SFNO_GEMM_GEOM = ("a_off", "a_sb", "a_m1", "a_sm", "a_sm2", "a_sk", "w_sb", "w_plane", "ldw", "o_off", "o_sb", "o_m1", "o_sm", "o_sm2", "o_sn",
                  "M", "N", "K", "batch", "act", "k_lo_step", "m_cap0", "m_cap_step", "a2_sk", "a2_k_split", "terms")


def _sfno_gemm(a, w, out, bias, res_pre, res_post, a_kscale, a_kshift, a2, geom) -> None:
    from .sfno import engine
    lib = engine.load_library()
    if len(geom) != len(SFNO_GEMM_GEOM):
        raise ValueError(f"sfno_gemm: geom has {len(geom)} entries, expected {len(SFNO_GEMM_GEOM)}")
    g = dict(zip(SFNO_GEMM_GEOM, geom))
    for t, what in ((a, "a"), (out, "out"), (bias, "bias"), (res_pre, "res_pre"), (res_post, "res_post"), (a_kscale, "a_kscale"), (a_kshift, "a_kshift"), (a2, "a2")):
        if t is not None:
            _f32(t, what, a.device)
    if w.dtype != torch.float16 or w.device != a.device:
        raise ValueError("sfno_gemm: w must be the fp16 hi/lo planes of sksfno_prepare_weight on the same device")
    d = engine.GemmDesc(_opt(a, 4 * g["a_off"]), g["a_sb"], g["a_m1"], g["a_sm"], g["a_sm2"], g["a_sk"],
                        w.data_ptr(), g["w_sb"], g["w_plane"], g["ldw"], _opt(bias), _opt(res_pre, 4 * g["o_off"]), _opt(res_post, 4 * g["o_off"]),
                        _opt(out, 4 * g["o_off"]), g["o_sb"], g["o_m1"], g["o_sm"], g["o_sm2"], g["o_sn"], g["M"], g["N"], g["K"], g["batch"], g["act"],
                        g["k_lo_step"], g["m_cap0"], g["m_cap_step"], _opt(a_kscale), _opt(a_kshift), _opt(a2), g["a2_sk"], g["a2_k_split"], g["terms"])
    with torch.cuda.device(a.device):
        native.check(lib.sksfno_gemm_run(ctypes.byref(d), native.stream(a.device)), "sksfno_gemm_run", lib)


def _sfno_instance_norm(x, gamma, beta, out, C: int, HW: int, eps: float) -> None:
    from .sfno import engine
    lib = engine.load_library()
    with torch.cuda.device(x.device):
        native.check(lib.sksfno_instance_norm(_f32(x, "x"), _f32(gamma, "gamma", x.device), _f32(beta, "beta", x.device), _f32(out, "out", x.device), C, HW, eps, native.stream(x.device)),
            "sksfno_instance_norm", lib)


def _sfno_chain(mode: int, shape: int, y, x, res, out, HW: int, C: int, KX: int, OUT: int, w1f, w2f, v1f, v2f, tab) -> None:
    from .sfno import engine
    lib = engine.load_library()
    dev = y.device
    for t, what in ((y, "y"), (x, "x"), (res, "res"), (out, "out"), (tab, "tab")):
        if t is not None:
            _f32(t, what, dev)
    for t, what in ((w1f, "w1f"), (w2f, "w2f"), (v1f, "v1f"), (v2f, "v2f")):
        if t is not None and (t.dtype != torch.float16 or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"sfno_chain: {what} must be the fp16 planes of sksfno_prepare_chain_weights on the same device")
    nin = KX if mode == engine.CHAIN_ENC else C
    nout = OUT if mode == engine.CHAIN_TAIL else C
    if y.numel() < nin * HW or res.numel() < C * HW or out.numel() < nout * HW or (x is not None and x.numel() < KX * HW):
        raise ValueError("sfno_chain: an activation tensor is smaller than channels x HW")
    d = engine.ChainDesc(mode, shape, y.data_ptr(), _opt(x), res.data_ptr(), out.data_ptr(), HW, C, KX, OUT, w1f.data_ptr(), w2f.data_ptr(),
                         _opt(v1f), _opt(v2f), tab.data_ptr())
    with torch.cuda.device(dev):
        native.check(lib.sksfno_chain_run(ctypes.byref(d), native.stream(y.device)), "sksfno_chain_run", lib)


def _sfno_instance_stats(x, gamma, beta, tab, shift_off: int, C: int, HW: int, eps: float) -> None:
    from .sfno import engine
    lib = engine.load_library()
    dev = x.device
    if tab.numel() < shift_off + C or x.numel() < C * HW:
        raise ValueError("sfno_instance_stats: tab or x too small")
    with torch.cuda.device(dev):
        native.check(lib.sksfno_instance_stats(_f32(x, "x"), _f32(gamma, "gamma", dev), _f32(beta, "beta", dev), _f32(tab, "tab", dev),
                                      ctypes.c_void_p(tab.data_ptr() + 4 * shift_off), C, HW, eps, native.stream(x.device)), "sksfno_instance_stats", lib)


# ---- GraphCast -------------------------------------------------------------------------------------------------------------- #
def _gc_gather_gemm(src, idx, width, w, w_plane: int, ldw: int, bias, out, M: int, N: int, act: int, kscale, kshift) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    if not (1 <= len(src) <= 3) or len(idx) != len(src) or len(width) != len(src):
        raise ValueError("gc_gather_gemm: 1..3 sources with one (optional) index tensor and one width each")
    d = engine.GatherDesc()
    dev = out.device
    for s, (t, ix, wd) in enumerate(zip(src, idx, width)):
        _f32(t, f"src[{s}]", dev)
        if ix is not None and (ix.dtype != torch.int32 or ix.device != dev or not ix.is_contiguous()):
            raise ValueError("gc_gather_gemm: index tensors are contiguous int32 on the same device")
        d.src[s], d.idx[s] = t.data_ptr(), (ix.data_ptr() if ix is not None else None)
        d.ld[s] = t.shape[-1] if t.dim() == 2 else wd
        d.width[s] = wd
    d.n_src = len(src)
    d.kscale, d.kshift = (kscale.data_ptr() if kscale is not None else None), (kshift.data_ptr() if kshift is not None else None)
    d.w, d.w_plane, d.ldw = w.data_ptr(), w_plane, ldw
    d.bias = _f32(bias, "bias", dev).value
    d.out, d.ldo, d.M, d.N, d.act = _f32(out, "out").value, N, M, N, act
    with torch.cuda.device(dev):
        native.check(lib.skgc_gather_gemm(ctypes.byref(d), native.stream(out.device)), "skgc_gather_gemm", lib)


def _gc_linear_layer_norm(a, lda: int, K: int, w, w_plane: int, ldw: int, bias, gamma, beta, res, out, rows: int) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = out.device
    with torch.cuda.device(dev):
        native.check(lib.skgc_linear_layer_norm(_f32(a, "a", dev), lda, K, ctypes.c_void_p(w.data_ptr()), w_plane, ldw, _f32(bias, "bias", dev), _f32(gamma, "gamma", dev),
                                       _f32(beta, "beta", dev), _opt(res), _f32(out, "out"), rows, native.stream(out.device)), "skgc_linear_layer_norm", lib)


def _gc_sum_linear_layer_norm(src, src_off, ld, idx, K: int, act: int, w, w_plane: int, ldw: int, bias, gamma, beta, res, out, rows: int, group: int = 0) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = out.device
    if not (1 <= len(src) <= 3) or not (len(src) == len(src_off) == len(ld) == len(idx)):
        raise ValueError("gc_sum_linear_layer_norm: 1..3 sources with an element offset, a leading dimension and an (optional) index tensor each")
    d = engine.SumDesc()
    for s, (t, off, l, ix) in enumerate(zip(src, src_off, ld, idx)):
        _f32(t, f"src[{s}]", dev)
        if ix is not None and (ix.dtype != torch.int32 or ix.device != dev or not ix.is_contiguous()):
            raise ValueError("gc_sum_linear_layer_norm: index tensors are contiguous int32 on the same device")
        d.src[s], d.idx[s], d.ld[s] = t.data_ptr() + 4 * off, (ix.data_ptr() if ix is not None else None), l
    d.n_src, d.K, d.act = len(src), K, act
    d.w, d.w_plane, d.ldw = w.data_ptr(), w_plane, ldw
    d.bias = bias.data_ptr() if bias is not None else None
    d.gamma, d.beta = _f32(gamma, "gamma", dev).value, _f32(beta, "beta", dev).value
    d.res = res.data_ptr() if res is not None else None
    d.out, d.rows, d.group = _f32(out, "out").value, rows, group
    with torch.cuda.device(dev):
        native.check(lib.skgc_sum_linear_layer_norm(ctypes.byref(d), native.stream(out.device)), "skgc_sum_linear_layer_norm", lib)


def _gc_layer_norm(x, gamma, beta, res, out, rows: int, N: int) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = out.device
    with torch.cuda.device(dev):
        native.check(lib.skgc_layer_norm(_f32(x, "x", dev), _f32(gamma, "gamma", dev), _f32(beta, "beta", dev), _opt(res), _f32(out, "out"), rows, N, native.stream(out.device)), "skgc_layer_norm", lib)


def _gc_segment_sum(e, offsets, out, acc, n_nodes: int, N: int) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = out.device
    if offsets.dtype != torch.int32 or offsets.device != dev:
        raise ValueError("gc_segment_sum: offsets are int32 on the same device")
    with torch.cuda.device(dev):
        native.check(lib.skgc_segment_sum(_f32(e, "e", dev), ctypes.c_void_p(offsets.data_ptr()), _f32(out, "out"), _opt(acc), n_nodes, N, native.stream(out.device)), "skgc_segment_sum", lib)


def _gc_edge_update(e_in, e_out, term, term_off, ld, idx, recv, w1f, w2f, b2, gamma, beta, agg, heads, rows: int, probe=None, w1_planes: int = 2) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = agg.device
    if len(term) > 2 or not (len(term) == len(term_off) == len(ld) == len(idx)):
        raise ValueError("gc_edge_update: at most two gathered terms, each with an element offset, a leading dimension and an index tensor")
    d = engine.EdgeDesc()
    d.e_in = _f16(e_in, "e_in", dev)
    d.e_out = _f16(e_out, "e_out", dev) if e_out is not None else None
    for s, (t, off, l, ix) in enumerate(zip(term, term_off, ld, idx)):
        _f32(t, f"term[{s}]", dev)
        d.term[s], d.idx[s], d.ld[s] = t.data_ptr() + 4 * off, _i32(ix, f"idx[{s}]", dev), l
        if ix.numel() < rows:
            raise ValueError("gc_edge_update: index tensors hold one entry per packed row")
    d.n_term = len(term)
    if recv.numel() < rows or e_in.numel() < rows * 512 or (e_out is not None and e_out.numel() < rows * 512):
        raise ValueError("gc_edge_update: recv / e_in / e_out are smaller than `rows` packed rows")
    d.recv = _i32(recv, "recv", dev)
    d.w1f = _f16(w1f, "w1f", dev) if w1f is not None else None
    d.w2f = _f16(w2f, "w2f", dev)
    d.b2, d.gamma, d.beta = _f32(b2, "b2", dev).value, _f32(gamma, "gamma", dev).value, _f32(beta, "beta", dev).value
    d.agg = _f32(agg, "agg").value
    if heads is not None:
        if heads.numel() < rows // 128 * 512:
            raise ValueError("gc_edge_update: heads holds one 512-wide row per 128-row tile")
    elif rows > 128 and bool(((recv[127:rows - 1:128] == recv[128:rows:128]) & (recv[128:rows:128] >= 0)).any().item()):
        # ad-hoc callers only (one blocking device read): GraphcastEngine.pack() proves the same thing on the host (fused.continuation_list,
        # padding rows -1 excluded there as here) and always hands over a heads buffer, so the engine's step never comes this way
        raise ValueError("gc_edge_update: a receiver's run continues across a tile boundary -- pass a heads buffer (and run gc_segment_fixup)")
    if agg.numel() < 512 or any(t.numel() - off < l for t, off, l in zip(term, term_off, ld)):
        raise ValueError("gc_edge_update: agg / term buffers are smaller than one row")
    d.heads = _f32(heads, "heads", dev).value if heads is not None else None
    d.rows, d.has_fc1, d.w1_planes = rows, int(w1f is not None), w1_planes
    if w1f is not None and w1f.numel() != w1_planes * 512 * 512:
        raise ValueError("gc_edge_update: w1f holds w1_planes planes of [512][512] in fragment order")
    d.probe = probe.data_ptr() if probe is not None else None
    with torch.cuda.device(dev):
        native.check(lib.skgc_edge_update(ctypes.byref(d), native.stream(agg.device)), "skgc_edge_update", lib)


def _gc_segment_fixup(agg, heads, nodes, first, tiles) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = agg.device
    with torch.cuda.device(dev):
        native.check(lib.skgc_segment_fixup(_f32(agg, "agg"), _f32(heads, "heads", dev), ctypes.c_void_p(_i32(nodes, "nodes", dev)), ctypes.c_void_p(_i32(first, "first", dev)),
                                   ctypes.c_void_p(_i32(tiles, "tiles", dev)), nodes.numel(), native.stream(agg.device)), "skgc_segment_fixup", lib)


def _gc_node_mlp(src, src_off, ld, w1f, w2f, b1, b2, gamma, beta, res, res_off: int, ld_res: int, out, out_off: int, ld_out: int, rows: int) -> None:
    from .graphcast import engine
    lib = engine.load_library()
    dev = out.device
    if not (1 <= len(src) <= 2) or not (len(src) == len(src_off) == len(ld)):
        raise ValueError("gc_node_mlp: one or two fp32 sources, each with an element offset and a leading dimension")
    d = engine.NodeDesc()
    for s, (t, off, l) in enumerate(zip(src, src_off, ld)):
        _f32(t, f"src[{s}]", dev)
        if t.numel() < off + (rows - 1) * l + 512:
            raise ValueError("gc_node_mlp: source smaller than rows x 512")
        d.src[s], d.ld[s] = t.data_ptr() + 4 * off, l
    d.n_src = len(src)
    d.w1f, d.w2f = _f16(w1f, "w1f", dev), _f16(w2f, "w2f", dev)
    if w1f.numel() != 2 * 512 * 512 * len(src) or w2f.numel() != 2 * 512 * 512:
        raise ValueError("gc_node_mlp: weight fragments are [512][512 n_src] and [512][512] with hi/lo planes")
    d.b1, d.b2 = _f32(b1, "b1", dev).value, _f32(b2, "b2", dev).value
    d.gamma, d.beta = _f32(gamma, "gamma", dev).value, _f32(beta, "beta", dev).value
    d.res = (_f32(res, "res", dev).value + 4 * res_off) if res is not None else None
    d.ld_res = ld_res
    if out.numel() < out_off + (rows - 1) * ld_out + 512:
        raise ValueError("gc_node_mlp: out smaller than rows x 512")
    d.out, d.ld_out, d.rows = _f32(out, "out").value + 4 * out_off, ld_out, rows
    with torch.cuda.device(dev):
        native.check(lib.skgc_node_mlp(ctypes.byref(d), native.stream(out.device)), "skgc_node_mlp", lib)


# ---- FourCastNet v1 ------------------------------------------------------------------------------------------------------------ #
def _fcn():
    from .fcn import engine
    return engine.load_library()


def _fcn_layer_norm(x, gamma, beta, out, rows: int, C: int, eps: float) -> None:
    lib = _fcn()
    dev = x.device
    if x.numel() < rows * C or out.numel() < rows * C:
        raise ValueError("fcn_layer_norm: x / out smaller than rows x C")
    with torch.cuda.device(dev):
        native.check(lib.skfcn_layer_norm(_f32(x, "x"), _f32(gamma, "gamma", dev), _f32(beta, "beta", dev), _f32(out, "out", dev), rows, C, eps, native.stream(x.device)),
            "skfcn_layer_norm", lib)


def _fcn_mlp(x, w1f, w2f, b1, b2, gamma, beta, out, rows: int, C: int, hidden: int, eps: float) -> None:
    from .fcn import engine
    lib = _fcn()
    dev = x.device
    if x.numel() < rows * C or out.numel() < rows * C or w1f.numel() != 2 * C * hidden or w2f.numel() != 2 * C * hidden:
        raise ValueError("fcn_mlp: tensor sizes do not match rows, C and hidden")
    d = engine.MlpDesc(_f32(x, "x").value, _f32(out, "out", dev).value, rows, C, hidden, _f32(gamma, "gamma", dev).value, _f32(beta, "beta", dev).value,
                       eps, _f16(w1f, "w1f", dev), _f16(w2f, "w2f", dev), _f32(b1, "b1", dev).value, _f32(b2, "b2", dev).value)
    with torch.cuda.device(dev):
        native.check(lib.skfcn_mlp_run(ctypes.byref(d), native.stream(x.device)), "skfcn_mlp_run", lib)


def _fcn_spectral_mlp(z, w1f, w2f, b1e, b2e, geom: list[int], lam: float) -> None:
    from .fcn import engine
    lib = _fcn()
    dev = z.device
    if len(geom) != 6:
        raise ValueError("fcn_spectral_mlp: geom = [rows, m1, sm, sm2, im_off, nblocks]")
    rows, m1, sm, sm2, im_off, nb = geom
    last = ((rows - 1) // m1) * sm2 + ((rows - 1) % m1) * sm + im_off + engine.SPECTRAL_BLOCK * nb
    if z.numel() < last or w1f.numel() != 2 * nb * 192 * 192 or w2f.numel() != 2 * nb * 192 * 192 or b1e.numel() != nb * 192 or b2e.numel() != nb * 192:
        raise ValueError("fcn_spectral_mlp: tensor sizes do not match the geometry")
    d = engine.SpectralMlpDesc(_f32(z, "z").value, rows, sm, sm2, im_off, m1, nb, _f16(w1f, "w1f", dev), _f16(w2f, "w2f", dev),
                               _f32(b1e, "b1e", dev).value, _f32(b2e, "b2e", dev).value, lam)
    with torch.cuda.device(dev):
        native.check(lib.skfcn_spectral_mlp(ctypes.byref(d), native.stream(z.device)), "skfcn_spectral_mlp", lib)


# ---- DLWP ---------------------------------------------------------------------------------------------------------------------- #
def _dlwp():
    from .dlwp import engine
    return engine, engine.load_library()


def _i32p(t, what: str, dev):
    return ctypes.c_void_p(_i32(t, what, dev))


def _dlwp_csr(ptr, col, S, rows: int, n_cols_src: int, dev, what: str):
    if ptr.numel() != rows + 1 or col.numel() != S.numel():
        raise ValueError(f"{what}: row_ptr must hold rows + 1 entries and col / S one per non-zero")
    return _i32p(ptr, f"{what}.row_ptr", dev), _i32p(col, f"{what}.col", dev), _f32(S, f"{what}.S", dev)


def _dlwp_ingest(x0, x1, center, inv_scale, row_ptr, col, S, lat, lon, statics, days0: float, days1: float, out, channels: int, ld_out: int) -> None:
    engine, lib = _dlwp()
    dev = out.device
    cells = row_ptr.numel() - 1
    points = x0.numel() // max(channels, 1)
    if x0.numel() != x1.numel() or x0.numel() != channels * points or out.numel() < cells * ld_out or lat.numel() != cells or lon.numel() != cells \
            or statics.numel() != 2 * cells or center.numel() != channels or inv_scale.numel() != channels:
        raise ValueError("dlwp_ingest: tensor sizes do not match channels, the map's rows and ld_out")
    if col.numel() and int(col.max()) >= points:
        raise ValueError("dlwp_ingest: map columns outside the state")
    for t, w in ((lat, "lat"), (lon, "lon")):
        if t.dtype != torch.float64 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"dlwp_ingest: {w} must be a contiguous float64 tensor on {dev}")
    rp, cl, sv = _dlwp_csr(row_ptr, col, S, cells, points, dev, "dlwp_ingest")
    d = engine.IngestDesc(_f32(x0, "x0", dev), _f32(x1, "x1", dev), _f32(center, "center", dev), _f32(inv_scale, "inv_scale", dev), rp, cl, sv,
                          lat.data_ptr(), lon.data_ptr(), _f32(statics, "statics", dev), days0, days1, _f32(out, "out", dev), channels, cells, points, ld_out)
    with torch.cuda.device(dev):
        native.check(lib.skdlwp_ingest(ctypes.byref(d), native.stream(dev)), "skdlwp_ingest", lib)


def _dlwp_conv(src0, src1, pad, w, w_plane: int, w_polar: int, ldw: int, bias, out, geom: list[int], slope: float, clamp_max: float) -> None:
    engine, lib = _dlwp()
    dev = out.device
    if len(geom) != 9:
        raise ValueError("dlwp_conv: geom = [n, c0, c1, mode0, taps, cout, ld_out, act, flip_face]")
    n, c0, c1, mode0, taps, cout, ld_out, act, flip = geom
    n0 = {0: n, 1: 2 * n, 2: n // 2}.get(mode0, n)
    if src0.numel() < 6 * n0 * n0 * c0 or (c1 and (src1 is None or src1.numel() < 6 * n * n * c1)) or out.numel() < 6 * n * n * ld_out \
            or pad.numel() != 48 or bias.numel() != 2 * cout or w.numel() < w_plane + w_polar + cout * ldw or w_polar < cout * ldw \
            or w_plane < w_polar + cout * ldw or ldw < taps * (c0 + c1):
        raise ValueError("dlwp_conv: tensor sizes do not match the geometry")
    faces, turns = pad.reshape(-1)[0::2], pad.reshape(-1)[1::2]
    if int(faces.min()) < 0 or int(faces.max()) > 5 or int(turns.min()) < 0 or int(turns.max()) > 3:
        raise ValueError("dlwp_conv: pad holds (face < 6, quarter turns < 4) pairs")
    d = engine.ConvDesc(_f32(src0, "src0", dev), _f32(src1, "src1", dev) if src1 is not None else None, _i32p(pad, "pad", dev), _f16(w, "w", dev),
                        w_plane, w_polar, ldw, _f32(bias, "bias", dev), _f32(out, "out", dev), n, c0, c1, mode0, taps, cout, ld_out, act, flip,
                        slope, clamp_max)
    with torch.cuda.device(dev):
        native.check(lib.skdlwp_conv(ctypes.byref(d), native.stream(dev)), "skdlwp_conv", lib)


def _dlwp_egress(y, row_ptr, col, S, center, scale, out6, out12, channels: int, ld_y: int) -> None:
    engine, lib = _dlwp()
    dev = y.device
    points = row_ptr.numel() - 1
    cells = y.numel() // max(ld_y, 1)
    if out6.numel() != channels * points or out12.numel() != channels * points or center.numel() != channels or scale.numel() != channels:
        raise ValueError("dlwp_egress: tensor sizes do not match channels and the map's rows")
    if col.numel() and int(col.max()) >= cells:
        raise ValueError("dlwp_egress: map columns outside the cube output")
    rp, cl, sv = _dlwp_csr(row_ptr, col, S, points, cells, dev, "dlwp_egress")
    d = engine.EgressDesc(_f32(y, "y", dev), rp, cl, sv, _f32(center, "center", dev), _f32(scale, "scale", dev), _f32(out6, "out6", dev),
                          _f32(out12, "out12", dev), channels, cells, points, ld_y)
    with torch.cuda.device(dev):
        native.check(lib.skdlwp_egress(ctypes.byref(d), native.stream(dev)), "skdlwp_egress", lib)


# ---- FuXi ---------------------------------------------------------------------------------------------------------------------- #
def _fuxi():
    from .fuxi import engine
    return engine, engine.load_library()


def _fuxi_layer_norm(x, res, gamma, beta, out, rows: int, C: int, eps: float) -> None:
    engine, lib = _fuxi()
    dev = out.device
    if x.numel() < rows * C or out.numel() < rows * C or (res is not None and res.numel() < rows * C) or gamma.numel() != C or beta.numel() != C:
        raise ValueError("fuxi_layer_norm: tensor sizes do not match rows and C")
    with torch.cuda.device(dev):
        native.check(lib.skfuxi_layer_norm(_f32(x, "x", dev), _f32(res, "res", dev) if res is not None else None, _f32(gamma, "gamma", dev),
                                           _f32(beta, "beta", dev), _f32(out, "out", dev), rows, C, eps, native.stream(dev)), "skfuxi_layer_norm", lib)


def _fuxi_window_attention(qkv, out, cpb, logit_scale, geom: list[int], mask_value: float, logit_max: float) -> None:
    engine, lib = _fuxi()
    dev = out.device
    if len(geom) != 9:
        raise ValueError("fuxi_window_attention: geom = [H, W, C, heads, wh, ww, sh, sw, mask_lon]")
    H, W, C, heads, wh, ww, sh, sw, mlon = geom
    if qkv.numel() != H * W * 3 * C or out.numel() != H * W * C or cpb.numel() != heads * (2 * wh - 1) * (2 * ww - 1) or logit_scale.numel() != heads:
        raise ValueError("fuxi_window_attention: tensor sizes do not match the geometry")
    d = engine.AttnDesc(_f32(qkv, "qkv", dev), _f32(out, "out", dev), _f32(cpb, "cpb", dev), _f32(logit_scale, "logit_scale", dev), H, W, C, heads,
                        wh, ww, sh, sw, mlon, mask_value, logit_max, 1e-12)
    with torch.cuda.device(dev):
        native.check(lib.skfuxi_window_attention(ctypes.byref(d), native.stream(dev)), "skfuxi_window_attention", lib)


def _fuxi_resample(src, mean, std, out, h_src: int, w_src: int, h_out: int, w_out: int, align_corners: bool) -> None:
    engine, lib = _fuxi()
    dev = out.device
    ch = mean.numel()
    if src.numel() != ch * h_src * w_src or out.numel() != ch * h_out * w_out or std.numel() != ch:
        raise ValueError("fuxi_resample: tensor sizes do not match the geometry")
    d = engine.ResampleDesc(_f32(src, "src", dev), _f32(mean, "mean", dev), _f32(std, "std", dev), _f32(out, "out", dev), ch, h_src, w_src, h_out, w_out,
                            int(align_corners))
    with torch.cuda.device(dev):
        native.check(lib.skfuxi_resample(ctypes.byref(d), native.stream(dev)), "skfuxi_resample", lib)


# ---- FengWu -------------------------------------------------------------------------------------------------------------------- #
def _fengwu():
    from .fengwu import engine
    return engine, engine.load_library()


def _fengwu_layer_norm(x, gamma, beta, out, rows: int, batch: int, C: int, eps: float) -> None:
    engine, lib = _fengwu()
    dev = out.device
    if x.numel() < batch * rows * C or out.numel() < batch * rows * C or gamma.numel() != batch * C or beta.numel() != batch * C:
        raise ValueError("fengwu_layer_norm: tensor sizes do not match rows, batch and C")
    d = engine.LnDesc(_f32(x, "x", dev).value, _f32(gamma, "gamma", dev).value, _f32(beta, "beta", dev).value, _f32(out, "out", dev).value,
                      rows, batch, C, 0, 0, 0, 0, eps)
    with torch.cuda.device(dev):
        native.check(lib.skfw_layer_norm(ctypes.byref(d), native.stream(dev)), "skfw_layer_norm", lib)


def _fengwu_window_attention(qkv, qkv_bias, table, out, geom: list[int], scale: float) -> None:
    """geom = [batch, Z, H, W, Zp, Hp, Wp, fz, fh, fw, wz, wh, ww, sz, sh, sw, types_z, types_y, C, heads] (include/skyrim_fengwu.h)."""
    engine, lib = _fengwu()
    dev = out.device
    if len(geom) != 20:
        raise ValueError("fengwu_window_attention: geom = [batch, Z, H, W, Zp, Hp, Wp, fz, fh, fw, wz, wh, ww, sz, sh, sw, types_z, types_y, C, heads]")
    batch, Z, H, W = geom[:4]
    wz, wh, ww = geom[10:13]
    tz, ty, C, heads = geom[16:]
    N = wz * wh * ww
    tsb = tz * ty * heads * N * N
    if qkv.numel() != batch * Z * H * W * 3 * C or out.numel() != batch * Z * H * W * C or qkv_bias.numel() != batch * 3 * C or table.numel() != batch * tsb:
        raise ValueError("fengwu_window_attention: tensor sizes do not match the geometry")
    d = engine.AttnDesc(_f32(qkv, "qkv", dev).value, _f32(qkv_bias, "qkv_bias", dev).value, _f32(table, "table", dev).value, _f32(out, "out", dev).value,
                        tsb, *geom, scale)
    with torch.cuda.device(dev):
        native.check(lib.skfw_window_attention(ctypes.byref(d), native.stream(dev)), "skfw_window_attention", lib)


# ---- ensembles ----------------------------------------------------------------------------------------------------------------- #
def _ens_perturb(x0, std, out, chan_stride: int, scale: float, seed: int, member_first: int) -> None:
    from . import ensemble
    ensemble.perturb(x0, std, out, chan_stride, scale, seed, member_first)


def _ens_stats(members, table, offset: int, n: int, mean, spread, min, max, exceed, thresholds, quant, levels) -> None:
    """``table``: ensemble.member_table(members), the device array of the members' pointers."""
    from . import ensemble
    ensemble.stats(list(members), table, offset, n, mean, spread, min, max, exceed, list(thresholds), quant, list(levels))


# ---- verification -------------------------------------------------------------------------------------------------------------- #
def _score_fields(members, table, truth, weights, out, workspace, flags: int, clim, counts, c0: int, nc: int) -> None:
    """``table``: ensemble.member_table(members); ``flags``: the groups of verify.DET / VAR / CRPS / ACC / RANK."""
    from . import verify
    verify.score(list(members), table, truth, weights, out, workspace, flags, clim, counts, c0, nc)


# ---- cyclone detection ---------------------------------------------------------------------------------------------------------- #
def _track_detect(members, table, channels, band, thresholds, h_msl, h_vort, h_wind, h_core, rowc, records, count, workspace) -> None:
    """``table``: ensemble.member_table(members); the tables and ``rowc`` are those of tracks.geometry on the device."""
    from . import tracks
    tracks.detect(list(members), table, list(channels), list(band), list(thresholds), h_msl, h_vort, h_wind, h_core, rowc, records, count,
                  workspace)


# ---- derived fields ------------------------------------------------------------------------------------------------------------- #
def _derive_fields(members, table, program, weights, out, rowc, edges) -> None:
    """``program`` / ``weights``: derived.encode(ops); ``rowc`` and ``edges``: derived.row_table on the device (vorticity, divergence)."""
    from . import derived
    derived.run(list(members), table, derived.decode(program, weights), out, rowc, tuple(edges) if len(edges) else (derived.EDGE_POLE,) * 2)


def _thermo_fields(members, table, program, params, out, surface) -> None:
    """``program`` / ``params``: thermo.encode(ops); ``surface``: the (H, W) surface geopotential on the device, or None."""
    from . import thermo
    thermo.run(list(members), table, thermo.decode(program, params), out, surface)


def _vert_fields(members, table, program, params, out, surface) -> None:
    """``program`` / ``params``: vertical.encode(ops); ``surface``: the (H, W) surface geopotential on the device, or None."""
    from . import vertical
    vertical.run(list(members), table, vertical.decode(program, params), out, surface)


# ---- regridding ------------------------------------------------------------------------------------------------------------------- #
def _regrid(members, table, channels, row_start, row_count, row_weight, col_start, col_count, col_weight, out) -> None:
    """The two tables: ``regrid.Tables.on(device)``; ``out``: (M, len(channels), Ho, Wo)."""
    from . import regrid
    regrid.run(list(members), table, list(channels), (row_start, row_count, row_weight), (col_start, col_count, col_weight), out)


# ---- event verification ----------------------------------------------------------------------------------------------------------- #
def _event_counts(members, table, truth, channels, n_thr, thresholds, counts, hy, hx, sums, workspace) -> None:
    """``thresholds``: the thresholds of all event channels one after the other, ``n_thr[e]`` of them for channel e."""
    from . import events
    if sum(n_thr) != len(thresholds) or len(n_thr) != len(channels):
        raise ValueError("event_counts: n_thr holds one count per channel and sums to len(thresholds)")
    split, at = [], 0
    for n in n_thr:
        split.append(list(thresholds[at:at + n]))
        at += n
    events.run(list(members), table, truth, list(channels), split, counts, list(hy), hx, sums, workspace)


# ---- time-window aggregates --------------------------------------------------------------------------------------------------------- #
def _agg_update(members, table, program, params, stamp: float, acc) -> None:
    """``program`` / ``params``: aggregate.encode(ops); ``stamp``: the lead time in hours; ``acc``: (M, D, H, W)."""
    from . import aggregate
    aggregate.run(list(members), table, aggregate.decode(program, params), acc, stamp)


# ---- neighbourhood fields ------------------------------------------------------------------------------------------------------------ #
def _nbr_fields(members, table, program, params, half, weights, out) -> None:
    """``program`` / ``params``: neighbourhood.encode(ops); ``half``: one int32 (H, 2 reach + 1) disc table per radius; ``weights``: float64
    (H); ``out``: (M, D, H, W)."""
    from . import neighbourhood
    neighbourhood.run(list(members), table, neighbourhood.decode(program, params), list(half), weights, out)


# ---- climate-relative extremes ---------------------------------------------------------------------------------------------------------- #
def _clim_extremes(members, table, channels, clim, levels, floor, sot_index, sot_frac, sot_ref, sot_base, prob_level, prob_below, efi, sot,
                   prob) -> None:
    """``clim``: (nf, Q, H, W); ``levels``: the Q probability levels; the four ``sot_*`` lists hold one entry per SOT request
    (climate.sot_request), ``prob_level`` / ``prob_below`` one per tail-odds request; include/skyrim_clim.h has the arithmetic."""
    from . import climate
    climate.run_extremes(list(members), table, list(channels), clim, list(levels), list(floor) or None,
                         list(zip(sot_index, sot_frac, sot_ref, sot_base)), list(zip(prob_level, prob_below)), efi, sot, prob)


def _clim_quantiles(samples, table, channels, levels, clim) -> None:
    """``clim``: (nf, Q, H, W), the ``levels`` (numpy's "linear" method) of the listed channels over the N samples."""
    from . import climate
    climate.run_quantiles(list(samples), table, list(channels), list(levels), clim)


# ---- packed member archives -------------------------------------------------------------------------------------------------------------- #
def _pack_range(members, table, channels, tab, workspace) -> None:
    """``tab``: archive.new_table(M, nc, device), the records of the listed channels; ``workspace``: uint8, archive.workspace_bytes."""
    from . import archive
    archive.run_range(list(members), table, list(channels), tab, workspace)


def _pack_quantize(members, table, channels, tab, out, member_stride_bytes) -> None:
    """``out``: uint8, the big-endian codes of member m from byte m * member_stride_bytes (even, >= 2 nc H W)."""
    from . import archive
    archive.run_quantize(list(members), table, list(channels), tab, out, member_stride_bytes)


def _pack_unpack(codes, tab, out) -> None:
    """``codes``: uint8, the big-endian image of (nc, H, W) codes; ``tab``: its nc records; ``out``: float32 (nc, H, W)."""
    from . import archive
    archive.run_unpack(codes, tab, out)


# ---- point extraction ------------------------------------------------------------------------------------------------------------------- #
def _point_gather(members, table, channels, records, out) -> None:
    """``records``: points.device_records(...), int32 (P, 8); ``out``: (M, len(channels), P) or (M, stride >= len(channels) P)."""
    from . import points
    points.run(list(members), table, list(channels), records, out)


# ---- ensemble scenarios ----------------------------------------------------------------------------------------------------------------- #
def _gram(members, table, truth, channels, region, lat_weight, out, workspace) -> None:
    """``region``: (j0, nj, i0, ni); ``out``: float64 (len(channels), M', M') or (len(channels), stride >= M'^2) with M' = M + (truth is not None); ``workspace``:
    scenarios.workspace_bytes(M', nc, nj, ni) bytes."""
    from . import scenarios
    scenarios.gram(list(members), table, truth, list(channels), list(region), lat_weight, out, workspace)


def _member_combine(members, table, channels, coef, b, out) -> None:
    """``coef``: float32 (K, M); ``b``: float32 (K,); ``out``: float32 (K, len(channels), H, W)."""
    from . import scenarios
    scenarios.combine(list(members), table, list(channels), coef, b, out)


# ---- zonal power spectra ------------------------------------------------------------------------------------------------------------------ #
def _zonal_spectra(members, table, truth, channels, bands, lat_weight, out, workspace) -> None:
    """``bands``: j0, j1 of every band, flattened; ``out``: float64 (len(channels), n_bands, 3 or 6, W // 2 + 1), 6 kinds with a truth;
    ``workspace``: spectra.workspace_bytes(M, H, W, nc, bands, truth) bytes."""
    from . import spectra
    bands = list(bands)
    if len(bands) % 2:
        raise ValueError("zonal_spectra: bands holds j0, j1 of every band")
    spectra.zonal(list(members), table, truth, list(channels), list(zip(bands[0::2], bands[1::2])), lat_weight, out, workspace)


# ---- breeding cycles ---------------------------------------------------------------------------------------------------------------------- #
def _breed_norms(y0, members, table, lat_weight, S, workspace) -> None:
    """``S``: float64 (M, C); ``workspace``: breeding.workspace_bytes(M, C, H, W) bytes."""
    from . import breeding
    breeding.norms(y0, list(members), table, lat_weight, S, workspace)


def _breed_apply(x0, y0, members, table, f, out, out_table) -> None:
    """``f``: float32 (M, C); ``out``: M states, ``out[m]`` may be ``members[m]``; ``out_table``: ensemble.member_table(out)."""
    from . import breeding
    breeding.apply(x0, y0, list(members), table, f, list(out), out_table)


# ---- spherical perturbations --------------------------------------------------------------------------------------------------- #
def _noise_coeffs(out, sigma, F: int, f_first: int, seed: int, member_first: int) -> None:
    """``sigma``: the device table sigma_l 2^e, lmax floats; ``out``: [members][lmax][lmax][2][F]."""
    from . import noise
    noise.coeffs(out, sigma, F, f_first, seed, member_first)


def _noise_apply(x0, y, g, out, chan_stride: int) -> None:
    from . import noise
    noise.apply(x0, y, g, out, chan_stride)


# ---- per-step stochastic perturbations ------------------------------------------------------------------------------------------ #
def _stoch_coeffs(out, sigma, F: int, f_first: int, seed: int, member_first: int, draw: int) -> None:
    """``noise_coeffs`` with the generator's fourth counter word 1 + ``draw``."""
    from . import stochastic
    stochastic.coeffs(out, sigma, F, f_first, seed, member_first, draw)


def _stoch_evolve(p, sigma, F: int, f_first: int, seed: int, member_first: int, draw: int, phi: float, psi: float) -> None:
    """``p``: the coefficient state, evolved in place; ``phi``, ``psi``: fp32 values."""
    from . import stochastic
    stochastic.evolve(p, sigma, F, f_first, seed, member_first, draw, phi, psi)


def _stoch_apply(xp, xn, r, y, gs, ga, lim: float, out, chan_stride: int) -> None:
    """``r`` with ``gs`` (and ``xp``), or ``y`` with ``ga``, may be None: that term is skipped.  ``out`` may be ``xn``."""
    from . import stochastic
    stochastic.apply(xp, xn, r, y, gs, ga, lim, out, chan_stride)


# ---- weather objects ---------------------------------------------------------------------------------------------------------------------- #
def _object_planes(channels, thresholds, directions, connectivity, scales):
    if not len(channels) == len(thresholds) == len(directions) == len(connectivity) == len(scales):
        raise ValueError("object planes: channels, thresholds, directions, connectivity and scales have one entry per plane")
    return list(zip(channels, thresholds, directions, connectivity, scales))


def _object_label(members, table, channels, thresholds, directions, connectivity, scales, periodic: bool, min_pixels: int, capacity: int,
                  labels, ids, n_found, workspace) -> None:
    """``labels``, ``ids``: int32 (M, P, H, W); ``n_found``: int32 (M, P); ``workspace``: objects.workspace_bytes(M, P, H, W) bytes."""
    from . import objects
    objects.label(list(members), table, _object_planes(channels, thresholds, directions, connectivity, scales), periodic, min_pixels, capacity,
                  labels, ids, n_found, workspace)


def _object_attributes(members, table, channels, thresholds, directions, connectivity, scales, capacity: int, labels, ids, n_found, row_tables,
                       col_tables, records) -> None:
    """``row_tables``: float64 (6, H); ``col_tables``: float64 (5, W); ``records``: uint8, (M, P, capacity) records of 128 bytes."""
    from . import objects
    objects.attributes(list(members), table, _object_planes(channels, thresholds, directions, connectivity, scales), capacity, labels, ids,
                       n_found, row_tables, col_tables, records)


def _object_probability(ids, keep, counts) -> None:
    """``keep``: uint8 (M, P, capacity + 1); ``counts``: int32 (P, H, W)."""
    from . import objects
    objects.probability(ids, keep, counts)


_SCHEMAS = [
    ("pangu_step(int ctx, Tensor x, Tensor(a!) out) -> ()", _pangu_step),
    ("pangu_patch_embed(int ctx, Tensor x, Tensor(a!) out) -> ()", _pangu_patch_embed),
    ("pangu_block(int ctx, int layer, int block, Tensor(a!) x) -> ()", _pangu_block),
    ("pangu_downsample(int ctx, Tensor x1, Tensor(a!) out) -> ()", _pangu_downsample),
    ("pangu_upsample(int ctx, Tensor x2, Tensor(a!) out) -> ()", _pangu_upsample),
    ("pangu_patch_recover(int ctx, Tensor skip, Tensor x4, Tensor(a!) out) -> ()", _pangu_patch_recover),
    ("sfno_gemm(Tensor a, Tensor w, Tensor(a!) out, Tensor? bias, Tensor? res_pre, Tensor? res_post, Tensor? a_kscale, Tensor? a_kshift, Tensor? a2, int[] geom) -> ()",
     _sfno_gemm),
    ("sfno_instance_norm(Tensor x, Tensor gamma, Tensor beta, Tensor(a!) out, int C, int HW, float eps) -> ()", _sfno_instance_norm),
    ("sfno_chain(int mode, int shape, Tensor y, Tensor? x, Tensor res, Tensor(a!) out, int HW, int C, int KX, int OUT, Tensor w1f, Tensor w2f, "
     "Tensor? v1f, Tensor? v2f, Tensor tab) -> ()", _sfno_chain),
    ("sfno_instance_stats(Tensor x, Tensor gamma, Tensor beta, Tensor(a!) tab, int shift_off, int C, int HW, float eps) -> ()", _sfno_instance_stats),
    ("gc_gather_gemm(Tensor[] src, Tensor?[] idx, int[] width, Tensor w, int w_plane, int ldw, Tensor bias, Tensor(a!) out, int M, int N, int act, "
     "Tensor? kscale, Tensor? kshift) -> ()", _gc_gather_gemm),
    ("gc_linear_layer_norm(Tensor a, int lda, int K, Tensor w, int w_plane, int ldw, Tensor bias, Tensor gamma, Tensor beta, Tensor? res, Tensor(a!) out, int rows) -> ()",
     _gc_linear_layer_norm),
    ("gc_sum_linear_layer_norm(Tensor[] src, int[] src_off, int[] ld, Tensor?[] idx, int K, int act, Tensor w, int w_plane, int ldw, Tensor? bias, Tensor gamma, "
     "Tensor beta, Tensor? res, Tensor(a!) out, int rows, int group=0) -> ()", _gc_sum_linear_layer_norm),
    ("gc_layer_norm(Tensor x, Tensor gamma, Tensor beta, Tensor? res, Tensor(a!) out, int rows, int N) -> ()", _gc_layer_norm),
    ("gc_segment_sum(Tensor e, Tensor offsets, Tensor(a!) out, Tensor(b!)? acc, int n_nodes, int N) -> ()", _gc_segment_sum),
    ("gc_edge_update(Tensor e_in, Tensor(c!)? e_out, Tensor[] term, int[] term_off, int[] ld, Tensor[] idx, Tensor recv, Tensor? w1f, Tensor w2f, Tensor b2, "
     "Tensor gamma, Tensor beta, Tensor(a!) agg, Tensor(b!)? heads, int rows, Tensor(d!)? probe=None, int w1_planes=2) -> ()", _gc_edge_update),
    ("gc_segment_fixup(Tensor(a!) agg, Tensor heads, Tensor nodes, Tensor first, Tensor tiles) -> ()", _gc_segment_fixup),
    ("gc_node_mlp(Tensor[] src, int[] src_off, int[] ld, Tensor w1f, Tensor w2f, Tensor b1, Tensor b2, Tensor gamma, Tensor beta, Tensor? res, int res_off, "
     "int ld_res, Tensor(a!) out, int out_off, int ld_out, int rows) -> ()", _gc_node_mlp),
    ("fcn_layer_norm(Tensor x, Tensor gamma, Tensor beta, Tensor(a!) out, int rows, int C, float eps) -> ()", _fcn_layer_norm),
    ("fcn_mlp(Tensor x, Tensor w1f, Tensor w2f, Tensor b1, Tensor b2, Tensor gamma, Tensor beta, Tensor(a!) out, int rows, int C, int hidden, "
     "float eps) -> ()", _fcn_mlp),
    ("fcn_spectral_mlp(Tensor(a!) z, Tensor w1f, Tensor w2f, Tensor b1e, Tensor b2e, int[] geom, float lam) -> ()", _fcn_spectral_mlp),
    ("dlwp_ingest(Tensor x0, Tensor x1, Tensor center, Tensor inv_scale, Tensor row_ptr, Tensor col, Tensor S, Tensor lat, Tensor lon, "
     "Tensor statics, float days0, float days1, Tensor(a!) out, int channels, int ld_out) -> ()", _dlwp_ingest),
    ("dlwp_conv(Tensor src0, Tensor? src1, Tensor pad, Tensor w, int w_plane, int w_polar, int ldw, Tensor bias, Tensor(a!) out, int[] geom, "
     "float slope, float clamp_max) -> ()", _dlwp_conv),
    ("dlwp_egress(Tensor y, Tensor row_ptr, Tensor col, Tensor S, Tensor center, Tensor scale, Tensor(a!) out6, Tensor(b!) out12, int channels, "
     "int ld_y) -> ()", _dlwp_egress),
    ("fuxi_layer_norm(Tensor x, Tensor? res, Tensor gamma, Tensor beta, Tensor(a!) out, int rows, int C, float eps) -> ()", _fuxi_layer_norm),
    ("fuxi_window_attention(Tensor qkv, Tensor(a!) out, Tensor cpb, Tensor logit_scale, int[] geom, float mask_value, float logit_max) -> ()",
     _fuxi_window_attention),
    ("fuxi_resample(Tensor src, Tensor mean, Tensor std, Tensor(a!) out, int h_src, int w_src, int h_out, int w_out, bool align_corners) -> ()",
     _fuxi_resample),
    ("fengwu_layer_norm(Tensor x, Tensor gamma, Tensor beta, Tensor(a!) out, int rows, int batch, int C, float eps) -> ()", _fengwu_layer_norm),
    ("fengwu_window_attention(Tensor qkv, Tensor qkv_bias, Tensor table, Tensor(a!) out, int[] geom, float scale) -> ()", _fengwu_window_attention),
    ("ens_perturb(Tensor x0, Tensor std, Tensor(a!) out, int chan_stride, float scale, int seed, int member_first) -> ()", _ens_perturb),
    ("ens_stats(Tensor[] members, Tensor table, int offset, int n, Tensor(a!)? mean, Tensor(b!)? spread, Tensor(c!)? min, Tensor(d!)? max, "
     "Tensor(e!)? exceed, float[] thresholds, Tensor(f!)? quant, float[] levels) -> ()", _ens_stats),
    ("score_fields(Tensor[] members, Tensor table, Tensor truth, Tensor weights, Tensor(a!)? out, Tensor(b!) workspace, int flags, Tensor? clim, "
     "Tensor(c!)? counts, int c0, int nc) -> ()", _score_fields),
    ("track_detect(Tensor[] members, Tensor table, int[] channels, int[] band, float[] thresholds, Tensor h_msl, Tensor h_vort, Tensor h_wind, "
     "Tensor? h_core, Tensor rowc, Tensor(a!) records, Tensor(b!) count, Tensor(c!) workspace) -> ()", _track_detect),
    ("derive_fields(Tensor[] members, Tensor table, int[] program, float[] weights, Tensor(a!) out, Tensor? rowc, int[] edges) -> ()", _derive_fields),
    ("thermo_fields(Tensor[] members, Tensor table, int[] program, float[] params, Tensor(a!) out, Tensor? surface) -> ()", _thermo_fields),
    ("vert_fields(Tensor[] members, Tensor table, int[] program, float[] params, Tensor(a!) out, Tensor? surface) -> ()", _vert_fields),
    ("regrid(Tensor[] members, Tensor table, int[] channels, Tensor row_start, Tensor row_count, Tensor row_weight, Tensor col_start, "
     "Tensor col_count, Tensor col_weight, Tensor(a!) out) -> ()", _regrid),
    ("event_counts(Tensor[] members, Tensor table, Tensor truth, int[] channels, int[] n_thr, float[] thresholds, Tensor(a!) counts, int[] hy, "
     "Tensor? hx, Tensor(b!)? sums, Tensor(c!)? workspace) -> ()", _event_counts),
    ("agg_update(Tensor[] members, Tensor table, int[] program, float[] params, float stamp, Tensor(a!) acc) -> ()", _agg_update),
    ("nbr_fields(Tensor[] members, Tensor table, int[] program, float[] params, Tensor[] half, Tensor weights, Tensor(a!) out) -> ()", _nbr_fields),
    ("point_gather(Tensor[] members, Tensor table, int[] channels, Tensor records, Tensor(a!) out) -> ()", _point_gather),
    ("gram(Tensor[] members, Tensor table, Tensor? truth, int[] channels, int[] region, Tensor lat_weight, Tensor(a!) out, "
     "Tensor(b!) workspace) -> ()", _gram),
    ("member_combine(Tensor[] members, Tensor table, int[] channels, Tensor coef, Tensor b, Tensor(a!) out) -> ()", _member_combine),
    ("zonal_spectra(Tensor[] members, Tensor table, Tensor? truth, int[] channels, int[] bands, Tensor lat_weight, Tensor(a!) out, "
     "Tensor(b!) workspace) -> ()", _zonal_spectra),
    ("breed_norms(Tensor y0, Tensor[] members, Tensor table, Tensor lat_weight, Tensor(a!) S, Tensor(b!) workspace) -> ()", _breed_norms),
    ("breed_apply(Tensor x0, Tensor y0, Tensor[] members, Tensor table, Tensor f, Tensor(a!)[] out, Tensor out_table) -> ()", _breed_apply),
    ("noise_coeffs(Tensor(a!) out, Tensor sigma, int F, int f_first, int seed, int member_first) -> ()", _noise_coeffs),
    ("noise_apply(Tensor x0, Tensor y, Tensor g, Tensor(a!) out, int chan_stride) -> ()", _noise_apply),
    ("stoch_coeffs(Tensor(a!) out, Tensor sigma, int F, int f_first, int seed, int member_first, int draw) -> ()", _stoch_coeffs),
    ("stoch_evolve(Tensor(a!) p, Tensor sigma, int F, int f_first, int seed, int member_first, int draw, float phi, float psi) -> ()",
     _stoch_evolve),
    ("stoch_apply(Tensor? xp, Tensor xn, Tensor? r, Tensor? y, Tensor? gs, Tensor? ga, float lim, Tensor(a!) out, int chan_stride) -> ()",
     _stoch_apply),
    ("object_label(Tensor[] members, Tensor table, int[] channels, float[] thresholds, int[] directions, int[] connectivity, float[] scales, "
     "bool periodic, int min_pixels, int capacity, Tensor(a!) labels, Tensor(b!) ids, Tensor(c!) n_found, Tensor(d!) workspace) -> ()", _object_label),
    ("object_attributes(Tensor[] members, Tensor table, int[] channels, float[] thresholds, int[] directions, int[] connectivity, float[] scales, "
     "int capacity, Tensor labels, Tensor ids, Tensor n_found, Tensor row_tables, Tensor col_tables, Tensor(a!) records) -> ()", _object_attributes),
    ("object_probability(Tensor ids, Tensor keep, Tensor(a!) counts) -> ()", _object_probability),
    ("clim_extremes(Tensor[] members, Tensor table, int[] channels, Tensor clim, float[] levels, float[] floor, int[] sot_index, "
     "float[] sot_frac, int[] sot_ref, int[] sot_base, int[] prob_level, bool[] prob_below, Tensor(a!)? efi, Tensor(b!)? sot, "
     "Tensor(c!)? prob) -> ()", _clim_extremes),
    ("clim_quantiles(Tensor[] samples, Tensor table, int[] channels, float[] levels, Tensor(a!) clim) -> ()", _clim_quantiles),
    ("pack_range(Tensor[] members, Tensor table, int[] channels, Tensor(a!) tab, Tensor(b!) workspace) -> ()", _pack_range),
    ("pack_quantize(Tensor[] members, Tensor table, int[] channels, Tensor tab, Tensor(a!) out, int member_stride_bytes) -> ()", _pack_quantize),
    ("pack_unpack(Tensor codes, Tensor tab, Tensor(a!) out) -> ()", _pack_unpack),
]
OP_NAMES = [s.split("(", 1)[0] for s, _ in _SCHEMAS]


def register() -> None:
    """Define the schemas and attach the CUDA (ROCm) implementations.  Idempotent; importing this module registers."""
    global _registered
    if _registered:
        return
    for schema, fn in _SCHEMAS:
        _lib.define(schema)
        _lib.impl(schema.split("(", 1)[0], fn, "CUDA")
    _registered = True


register()
hip = getattr(torch.ops, _NS)
