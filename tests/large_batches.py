"""Batch-sized device arrays of the batched entry families, and the large-batch cases derived from them (data and arithmetic
only: importable without a device).

Every size below restates the host code that creates the array -- fsgm_epi_plan_create_sampling, epi_ensure_cost_buffers,
ensure_agg_buffers and the *_bytes helpers of epi_sweep.hip / epi_band.hip for the epipolar plan (capi_epi.hip), sgm_run_device
(capi_sgm.hip) for sgm(C), post_plan_create_batch (capi_post.hip) for the post-processing chain, hints_enqueue (capi_pyramid.hip) for the level
hints -- and none comes from a run.  A case names one array and one mark (2^31, 2^32 or 2^34 bytes) and derives the smallest batch
N such that (a) the array's N frames exceed the mark, (b) the mark falls strictly inside a frame, (c) at least two whole frames lie
beyond it; (d) the call's peak -- the plan's arrays, the caller's tensors and the reference side -- stays under CAP.
tests/test_large_batches_cpu.py asserts (a)-(d); tests/test_gpu_large_batches.py runs the cases."""
from collections import namedtuple

MARK31, MARK32, MARK34 = 1 << 31, 1 << 32, 1 << 34
GIB = 1 << 30
CAP = 64 * GIB
HEADROOM = 8 * GIB                     # a GPU case skips unless its peak plus this is free

# name in the plan / the call, bytes per frame, bytes of the element the kernels index it in (1 u8, 2 u16, 4 dword, 8 f64 / uint2, 16 uint4)
Array = namedtuple("Array", "name bytes_per_frame unit")

HP_TC = 8                              # epi_sweep.hip FSGM_HP_TC: checkpoint spacing of the pair kernels
BAND_WAVES = 8                         # epi_band.hip FSGM_BAND_WAVES
LINE_PIPES = ("packed16/nowrap", "packed16/wrap", "packed16/exact", "generic", "generic/exact")


def packed_lpp(D):
    """agg_packed_lpp: lanes per pixel at 16 costs a lane, 0 unless D = 16 << k, k <= 4"""
    return D // 16 if D in (16, 32, 64, 128, 256) else 0


def pair_ckpt_bytes(W, H, D, axis):
    length, lines = (H, W) if axis else (W, H)
    nt = (length + HP_TC - 1) // HP_TC
    return lines * (nt - 1 if nt > 1 else 1) * D


def band_rows(D):
    lpp = packed_lpp(D)
    return BAND_WAVES * (64 // lpp) if lpp else 0


def epi_plan_arrays(W, H, D, paths, pipeline, *, cost_stage=False, rectified=False, fb_check=False, runner_up=False, guide=False):
    """The batch-sized arrays of an fsgm_epi_plan that runs `pipeline` (EpiPlan.kernel_name's names)"""
    NP, N, lpp = W * H, W * H * D, packed_lpp(D)
    a = [Array("dC", N, 1), Array("dBestD", NP * 4, 4), Array("dMinC", NP * 4, 4)]
    if not rectified:
        a.append(Array("dOff", NP * 8, 8))
    if fb_check:
        a += [Array("dD2enc", NP * 4, 4), Array("dD2", NP * 4, 4), Array("dConf", NP, 1)]
    if runner_up:
        a.append(Array("dMinC2", NP * 4, 4))
    if cost_stage or fb_check:                                   # epi_ensure_cost_buffers
        a += [Array("dI1", NP, 1), Array("dI2", NP, 1), Array("dCen1", NP * 4, 4), Array("dCen2", NP * 4, 4), Array("dCraw", N, 1)]
        if not rectified:
            a += [Array("dPd0", NP * 16, 8), Array("dNd", NP * 16, 8)]
    elif guide:                                                  # epi_ensure_image_buffers
        a += [Array("dI1", NP, 1), Array("dI2", NP, 1)]
    lines = pipeline in LINE_PIPES
    pairs = pipeline == "pairs16/nowrap"
    sweep = pipeline in ("sweep16/nowrap", "sweep16par/nowrap", "sweep16mid/nowrap")
    par = pipeline in ("sweep16par/nowrap", "sweep16mid/nowrap")
    band = pipeline in ("band16/nowrap", "band16chain/nowrap")
    assert lines or pairs or sweep or band, pipeline
    if lines:
        a.append(Array("dL", N * paths, 1))
    else:
        a += [Array("dRec", NP * 8, 8), Array("dS0", NP * 2, 2)]
    if pairs or sweep:
        a += [Array("dLh", N, 1), Array("dCkpt", pair_ckpt_bytes(W, H, D, 0), 1)]
    if pairs:
        a.append(Array("dCkptV", pair_ckpt_bytes(W, H, D, 1), 1))
    if sweep or band:
        a.append(Array("dX", N, 1))
    if sweep:
        a.append(Array("dState", 2 * 3 * W * D, 1))
    if par:                                                      # (dLx: batches of up to 5 frames only)
        a += [Array("dXupAll", N, 1), Array("dStateUp", 2 * 3 * W * D, 1)]
    if band:
        R = band_rows(D)
        nbands = (H + R - 1) // R
        maps = max(nbands - 1, 1) if pipeline == "band16chain/nowrap" else 1
        a.append(Array("dBandEdge", maps * W * (3 if paths == 8 else 1) * lpp * 16, 16))
        if paths == 8:
            a.append(Array("dBits", NP * lpp * 4, 4))
    return a


def post_plan_arrays(W, H, staging=False):
    """fsgm_post_plan of a batch (post_plan_create_batch; ensure_staging for the host forms)"""
    NP = W * H
    a = [Array(n, NP * 8, 8) for n in ("dA", "dB", "dD2")] + [Array(n, NP * 4, 4) for n in ("dParent", "dSize", "dLeft")]
    if staging:
        a += [Array(n, NP * 8, 8) for n in ("dIn", "dOut", "dDisp", "dO")] + [Array("dPd0", NP * 16, 8), Array("dNd", NP * 16, 8)]
    return a


def pyd_plan_arrays(W, H, Sx, Sy, *, images=False, flow=False):
    """fsgm_pyd_plan of a batch (capi_pyd.hip fsgm_pyd_plan_create): the 2-D matcher's volumes in padded rows, RS = Sy rounded up to
    4 while both sides are <= 11 (pyd_kernels.h pyd_row_stride), PS = Sx * RS; dL holds 8 path volumes whatever the path count.
    images: the cost stage's (a pyramid level); flow: dFlow of sgm2d(return_flow) (capi_sgm2d.hip)."""
    NP = W * H
    rows = Sx <= 11 and Sy <= 11
    PS = Sx * (4 * ((Sy + 3) // 4) if rows else Sy)
    a = [Array("dC", NP * PS, 1), Array("dL", NP * PS * 8, 1), Array("dMv", NP * 16, 8), Array("dBestD", NP * 4, 4),
         Array("dMinC", NP * 4, 4), Array("dMvSub", NP * 16, 8)]
    if rows:
        a.append(Array("dDesc", NP * 32, 4))
    if images:
        a += [Array("dI1", NP, 1), Array("dI2", NP, 1), Array("dCen1", NP * 4, 4), Array("dCen2", NP * 4, 4)]
    if flow:
        a.append(Array("dFlow", NP * 16, 8))
    return a


def pyramid_arrays(W, H, levels, Sx=11, Sy=11):
    """fsgm_pyramid_plan of a batch of gray pairs: one fsgm_pyd_plan per level (capi_pyramid.hip create_levels) and the level's
    flow (pyramid_driver.h dFlow), level l at ceil(W / 2^l) x ceil(H / 2^l); names carry the level"""
    out = []
    for l in range(levels):
        w, h = -(-W // (1 << l)), -(-H // (1 << l))
        out += [Array(f"{a.name}[{l}]", a.bytes_per_frame, a.unit) for a in pyd_plan_arrays(w, h, Sx, Sy, images=True)]
        out.append(Array(f"dFlowLevel[{l}]", w * h * 16, 8))
    return out


def flow_pp_arrays(W, H):
    """fsgm_flow_pp_plan of a batch (capi_flow_pp.hip:66-70): the host forms' staging and scratch"""
    NP = W * H
    return [Array("dS", NP * 32, 8), Array("dC", NP * 16, 8), Array("dParent", NP * 8, 4), Array("dSize", NP * 8, 4), Array("dLeft", NP * 4, 4)]


def stereo_pp_arrays(W, H):
    """fsgm_stereo_pp_plan of a batch (capi_stereo_pp.hip:107-135)"""
    NP = W * H
    return [Array("dW", NP * 8, 8), Array("dDisp", NP * 4, 4), Array("dMinC", NP * 4, 4), Array("dI1", NP, 1), Array("dI2", NP, 1),
            Array("dPP", NP * 8, 8), Array("dChecked", NP * 8, 8), Array("dDisp2", NP * 8, 8)]


# What the inventory found for each batched entry family: "arrays" -- it has batch-sized device arrays and at least one case;
# "per-frame" -- nothing of it grows with the batch.
FAMILIES = {
    "epi_plan/fused": ("arrays", "EpiPlan upload_cost -> run -> download, the fused pipelines (capi_epi.hip ensure_agg_buffers)"),
    "epi_plan/lines": ("arrays", "EpiPlan on the line kernels: dL = paths volumes a frame"),
    "epi_plan/generic": ("arrays", "EpiPlan at a dMax outside the line classes: agg_generic_kernel, wta_generic_kernel"),
    "epi_plan/cost": ("arrays", "the cost stage from images: stereo_sgm, calc_cost_sgm_batch (epi_ensure_cost_buffers)"),
    "sgm_device": ("arrays", "torch_ops.sgm: the caller's volumes and the cached plan's (sgm_run_device)"),
    "ingest_hwd": ("arrays", "launch_sgm_ingest's hwd copy in launches of 2^34 bytes (sgm_ingest.hip)"),
    "sgm2d_device": ("arrays", "torch_ops.sgm2d: the caller's volumes and the cached fsgm_pyd_plan's (capi_sgm2d.hip, capi_pyd.hip:93-106)"),
    "post": ("arrays", "epi_postprocess on a batch of maps (post_plan_create_batch); n_frames * W * H >= 2^31 is refused at the entry"),
    "flow_pp": ("arrays", "flow_fb_check on the caller's tensors; flow_speckle_filter / flow_in_fill host forms through the cached "
                          "fsgm_flow_pp_plan (2 * n_frames * W * H >= 2^31 refused)"),
    "stereo_pp": ("arrays", "uniqueness_filter and stereo_fb_check on the caller's maps (stereo_pp_kernels.hip); the whole of "
                            "stereo_sgm_pp with maps across 2^32 bytes is above the cap (stereo_sgm_pp_peak)"),
    "level_hints": ("arrays", "flow_level_hints: launch_pyr_upsample2 / launch_pyr_median_upsample2 on the caller's tensors"),
    "pyramids": ("arrays", "pyramidal_sgm / pyramidal_sgm_ng on a batch: every level is a plan of the whole batch (capi_pyramid.hip "
                           "create_levels, capi_ng_pyramid.hip:52-58)"),
    "sum_tap": ("per-frame", "S of fsgm_sgm_device / download_sum: one frame through dS at a time (capi_sgm.hip sgm_run_device "
                             "'S never exists for a batch', capi_epi.hip epi_ensure_tap_buffers allocates p->N * 4)"),
}

Case = namedtuple("Case", "id family W H D paths pipeline n target target_bpf mark arrays caller_bytes ref_bytes sub_batch")


def frames_for(bytes_per_frame, mark):
    """Smallest batch whose array of bytes_per_frame a frame has the mark strictly inside frame k and frames k + 1, k + 2 beyond it"""
    return mark // bytes_per_frame + 3


def total(arrays, n):
    return sum(a.bytes_per_frame for a in arrays) * n


def sub_batch(arrays, extra=()):
    """Largest batch at which every listed array (and the caller's, `extra`: bytes per frame) stays below 2^31 bytes"""
    return (MARK31 - 1) // max([a.bytes_per_frame for a in arrays] + list(extra))


def peak(case):
    """(d): the plan's arrays, the caller's tensors and the reference side while the call under test is resident"""
    return total(case.arrays, case.n) + case.caller_bytes + case.ref_bytes


def crossings(case):
    """For every array of the case that exceeds 2^31 bytes: (name, bytes, exceeds 2^32 bytes, element index exceeds 2^31)"""
    out = []
    for a in case.arrays:
        b = a.bytes_per_frame * case.n
        if b > MARK31:
            out.append((a.name, b, b > MARK32, b // a.unit > MARK31))
    return out


def _case(id, family, W, H, D, paths, pipeline, target, mark, arrays, caller_per_frame, ref_per_frame, target_bpf=None, sub_cap=None):
    """target: an array of `arrays`, or the name of the caller's tensor with target_bpf its bytes per frame.  caller_per_frame:
    device bytes of the caller's tensors; ref_per_frame: of the reference outputs kept on the device for the comparison."""
    if target_bpf is None:
        target_bpf = {a.name: a for a in arrays}[target].bytes_per_frame
    n = frames_for(target_bpf, mark)
    sb = sub_batch(arrays, (caller_per_frame, target_bpf))
    sb = min(sb, sub_cap) if sub_cap else sb
    # the reference side: one sub-batch's arrays (its plan stays cached while the large call runs) and every frame's outputs
    ref = total(arrays, min(sb, n)) + ref_per_frame * n
    return Case(id, family, W, H, D, paths, pipeline, n, target, target_bpf, mark, tuple(arrays), caller_per_frame * n, ref, sb)


# One small odd frame for every case that leaves the shape open: W * H = 21513 = 3 * 71 * 101 has no factor 2, so a frame of any
# array here holds 2^k * odd bytes with k far below 31 and no frame boundary falls on a mark.
W0, H0 = 213, 101
FUSED = {8: {2: "sweep16/nowrap", 3: "sweep16par/nowrap", 4: "band16/nowrap", 5: "band16chain/nowrap", 6: "sweep16mid/nowrap"},
         4: {2: "pairs16/nowrap", 4: "band16/nowrap", 5: "band16chain/nowrap"}}


def _outputs(W, H, k=2):
    return W * H * 4 * k                                         # bestD, minC (and minC2 ...) of a frame


def cases():
    out = []
    NP = W0 * H0
    # 1. resident plan, fused pipelines, dC across 2^32 (host volumes: the caller holds nothing on the device)
    for paths, modes in FUSED.items():
        for mode, pipe in modes.items():
            out.append(_case(f"fused-p{paths}-m{mode}", "epi_plan/fused", W0, H0, 128, paths, pipe, "dC", MARK32,
                             epi_plan_arrays(W0, H0, 128, paths, pipe), 0, 0))
    # 2. line kernels: dL across 2^32 with dC below it (8 paths), dC itself across (4 paths)
    out.append(_case("lines-p8-L", "epi_plan/lines", W0, H0, 128, 8, "packed16/nowrap", "dL", MARK32,
                     epi_plan_arrays(W0, H0, 128, 8, "packed16/nowrap"), 0, 0))
    out.append(_case("lines-p4-C", "epi_plan/lines", W0, H0, 128, 4, "packed16/nowrap", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 128, 4, "packed16/nowrap"), 0, 0))
    out.append(_case("lines-p4-C-wrap", "epi_plan/lines", W0, H0, 128, 4, "packed16/wrap", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 128, 4, "packed16/wrap"), 0, 0))
    # 3. generic kernels
    out.append(_case("generic-d300", "epi_plan/generic", W0, H0, 300, 4, "generic", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 300, 4, "generic"), 0, 0))
    # 4. the cost stage writing dC across 2^32 from images (rectified: stereo_sgm; vz: calc_cost_sgm_batch)
    out.append(_case("cost-stereo-d256", "epi_plan/cost", W0, H0, 256, 4, "pairs16/nowrap", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 256, 4, "pairs16/nowrap", cost_stage=True, rectified=True, fb_check=True), 0, 0))
    out.append(_case("cost-stereo-d256-ru", "epi_plan/cost", W0, H0, 256, 4, "packed16/nowrap", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 256, 4, "packed16/nowrap", cost_stage=True, rectified=True, runner_up=True), 0, 0))
    out.append(_case("cost-stereo-d260", "epi_plan/cost", W0, H0, 260, 4, "generic", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 260, 4, "generic", cost_stage=True, rectified=True), 0, 0))
    out.append(_case("cost-vz-d128", "epi_plan/cost", W0, H0, 128, 4, "pairs16/nowrap", "dC", MARK32,
                     epi_plan_arrays(W0, H0, 128, 4, "pairs16/nowrap", cost_stage=True), 0, 0))
    # 5. torch_ops.sgm: the caller's (N, D, H, W) / (N, H, W, D) tensor across 2^32, read where it lies
    for id, pipe, kw in (("sgm-dhw", "pairs16/nowrap", {}), ("sgm-hwd", "pairs16/nowrap", {}),
                         ("sgm-dhw-exact", "packed16/exact", {}), ("sgm-hwd-ru", "packed16/nowrap", {"runner_up": True}),
                         ("sgm-dhw-adaptive", "packed16/nowrap", {"guide": True}), ("sgm-hwd-wrap", "packed16/wrap", {})):
        D = 64
        arrays = epi_plan_arrays(W0, H0, D, 4, pipe, **kw)
        k = 3 if kw.get("runner_up") else 2
        caller = NP * D + _outputs(W0, H0, k) + (NP if kw.get("guide") else 0)
        out.append(_case(id, "sgm_device", W0, H0, D, 4, pipe, "C", MARK32, arrays, caller, _outputs(W0, H0, k), target_bpf=NP * D))
    # 5b. the hwd copy's second launch: a source above 2^34 bytes.  torch_ops.sgm itself does not fit the cap there (see
    # sgm_over_2_34_peak), so the case runs the same launcher through EpiPlan.ingest_cost and reads dC back.
    W1, H1, D1 = 1241, 375, 16
    arrays = [a for a in epi_plan_arrays(W1, H1, D1, 4, "packed16/nowrap") if a.name != "dL"]   # no run: no aggregation buffers
    out.append(_case("ingest-hwd-2^34", "ingest_hwd", W1, H1, D1, 4, "none", "dC", MARK34, arrays, W1 * H1 * D1, 0))
    # 6. torch_ops.sgm2d: (N, 81, H, W) / (N, H, W, 81) across 2^32, the padded destination 108 bytes a pixel
    for id in ("sgm2d-dhw_yx", "sgm2d-hwd", "sgm2d-dhw_yx-exact"):
        arrays = pyd_plan_arrays(W0, H0, 9, 9, flow=True)
        caller = NP * (81 + 4 + 4 + 16 + 16 + 16)                # costs, bestD, minC, mvSub, flow, hints
        # (fsgm_sgm2d_last_kernel's names: 9 x 9 candidates inside the no-wrap budget take the row-packed aggregation)
        out.append(_case(id, "sgm2d_device", W0, H0, 81, 8, "generic/exact" if id.endswith("exact") else "rows", "costs", MARK32, arrays,
                         caller, NP * 40, target_bpf=NP * 81, sub_cap=16))
    # 7. post-processing on f64 maps across 2^32 bytes with n * W * H below 2^31 pixels (the reference outputs of a sub-batch are
    # compared and dropped before the next)
    caller = NP * (8 + 16 + 16 + 8 + 8 + 8 + 8)                  # D1, Pd0, nd, O, filterD1, filterD2, disp
    out.append(_case("post-chain", "post", W0, H0, 0, 0, "none", "dA", MARK32, post_plan_arrays(W0, H0), caller, 0, sub_cap=2048))
    # (caller: f, b, out and the index tensors of the tiling that torch's allocator keeps)
    out.append(_case("flow-fb-check", "flow_pp", W0, H0, 0, 0, "none", "f", MARK32, [], NP * 64, NP * 16, target_bpf=NP * 16))
    for id in ("flow-speckle", "flow-in-fill"):                  # host forms: the plan's staging dS holds [2][n][NP] twice
        out.append(_case(id, "flow_pp", W0, H0, 0, 0, "none", "dC", MARK32, flow_pp_arrays(W0, H0), NP * 16, 0))
    # (caller: the maps, costs and outputs, 24 bytes a pixel, and the temporaries of the seeded draws that torch's allocator keeps:
    # the first run measured 90 bytes a pixel in all)
    out.append(_case("uniqueness", "stereo_pp", W0, H0, 0, 0, "none", "map", MARK32, [], NP * 96, NP * 8, target_bpf=NP * 8))
    out.append(_case("stereo-fb-check", "stereo_pp", W0, H0, 0, 0, "none", "D1", MARK32, [], NP * 96, NP * 16, target_bpf=NP * 8))
    # 8. the pyramid drivers: level 1's dL (8 path volumes of 11 x 12 padded candidates) across 2^32; the neighbour-guided driver
    # runs the same batch (its level arena: capi_ng.hip ng_level_bufs)
    for id in ("pyramid-pyd", "pyramid-ng"):
        out.append(_case(id, "pyramids", W0, H0, 121, 8, id, "dL[0]", MARK32, pyramid_arrays(W0, H0, 3), NP * (2 + 16 + 4), NP * 20))
    # 8b. the level-hint kernels: next (N, 2, 2H, 2W) f64 across 2^32 bytes
    for id, size in (("hints-plain", 0), ("hints-median3", 3)):
        # (the reference side: the sub-batch results and their concatenation)
        out.append(_case(id, "level_hints", W0, H0, 0, 0, f"median{size}", "next", MARK32, [], NP * 16 + NP * 64, 2 * NP * 64,
                         target_bpf=NP * 64))
    return out


def sgm_over_2_34_peak(W=1241, H=375, D=16, paths=4):
    """Peak of torch_ops.sgm on an hwd tensor above 2^34 bytes in its cheapest pipeline (band sweeps, 4 paths): source, dC, dX,
    records and outputs -- above CAP, which is why case ingest-hwd-2^34 stops after the copy"""
    n = frames_for(W * H * D, MARK34)
    return (total(epi_plan_arrays(W, H, D, paths, "band16/nowrap"), n) + (W * H * D + _outputs(W, H)) * n)


def stereo_sgm_pp_peak(W=W0, H=H0, D=16):
    """Peak of stereo_sgm_pp with its f64 maps across 2^32 bytes at the smallest D of the fused cost stage: the rectified plan
    with fb_check (pair pipeline), the chain's plan and the five outputs -- above CAP, which is why family stereo_pp runs the
    chain's kernels on the caller's maps instead"""
    n = frames_for(W * H * 8, MARK32)
    epi = epi_plan_arrays(W, H, D, 4, "pairs16/nowrap", cost_stage=True, rectified=True, fb_check=True)
    return total(epi, n) + total(stereo_pp_arrays(W, H), n) + W * H * (2 + 8 + 8 + 4 + 4 + 8) * n
