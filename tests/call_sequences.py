"""Seeded sequences of one-shot calls that share the library's cached plans (PlanCache, fsgm_amd/csrc/capi_common.h), for
tests/test_call_sequences_cpu.py (the draws alone) and tests/test_gpu_call_sequences.py (the calls, one after the other, each on
the plan its predecessor left behind).

First the epi family: everything behind g_epi (cached_plan, fsgm_amd/csrc/capi_epi.hip; its callers in capi_epi.hip, capi_stereo.hip, capi_sgm.hip and capi_epi_driver.hip); the other caches follow below it.  A step is a Step tuple: the entry form, the shape and the
batch, the parameters that are part of the cache key, the ones that are not, what it asks back and the seed of its data.  Each
function consumes its RandomState in a fixed order; the order is part of the test suite's definition (tests/fuzz_configs.py).

A step's inputs and expected outputs are functions of the step alone (inputs, expected: memoised on it, never taken from a GPU
answer), and so is the pipeline a fresh plan would choose for it (pipeline)."""
import collections
import functools

import numpy as np

from fsgm_amd import epi, synth
from tests import budget_volumes as BV

EPI_CAP = 4                                                     # g_epi
EPI_SHAPES = [(37, 21, 32), (13, 26, 64), (61, 9, 16), (19, 13, 48), (23, 9, 144)]     # packed, packed, packed, split, generic
FUSABLE_D = (16, 32, 64, 128, 256)                              # agg_packed_lpp(D) != 0: what the fused pipelines take
LINE_D = FUSABLE_D + (48, 96, 192, 80, 160, 112, 224)           # agg_line_split(D): every other D runs the generic kernels
PENALTIES = [(6, 64), (100, 200), (0, 0), (21, 64), (22, 64), (63, 64)]
VMAX = (0.3, 0.5, 0.125)
D_MIN = (None, 0, -17, 7)
VOL_CMAX = (24, 255)
COST_BOUND = (24, 127, 255)
SAMPLING_VZ, SAMPLING_LINEAR, SAMPLING_RECTIFIED = 0, 1, 2

# entry forms -> the family whose code sets the plan up (what "the previous user was a different family" compares)
FAMILY = {"calc_cost_sgm": "calc_cost_sgm", "calc_cost_sgm_mex": "calc_cost_sgm", "calc_cost_sgm_linear": "linear",
          "stereo_sgm": "stereo", "sgm": "sgm", "sgm_batch": "sgm_batch", "sgm_torch": "sgm_batch"}

Step = collections.namedtuple("Step", [
    "form", "W", "H", "D", "batch",
    "paths", "vz", "adaptive", "agg_mode", "direction",         # key parameters (with the form's sampling; fb_check is 0 throughout)
    "P1", "P2", "subpixel", "vMax", "d_min", "vol_cmax", "cost_bound", "guide",      # non-key parameters
    "want_S", "want_C",                                         # requested outputs
    "seed",                                                     # of the step's data
    "refuse",                                                   # None, or why the library must refuse the call (status 1)
])


def rng(seed):
    return np.random.RandomState(7000 + seed)                   # only picks steps; data comes from synth


def key(s):
    """cached_plan's key: W, H, D, batch, paths, fb_check, vz_to_disp, sampling, direction, adaptive, agg_mode"""
    sampling = {"calc_cost_sgm_linear": SAMPLING_LINEAR, "stereo_sgm": SAMPLING_RECTIFIED}.get(s.form, SAMPLING_VZ)
    direction = s.direction if s.form == "stereo_sgm" else 0
    vz = s.vz if FAMILY[s.form] == "calc_cost_sgm" else 0
    adaptive = 0 if s.form == "sgm" else s.adaptive
    agg_mode = s.agg_mode if FAMILY[s.form] == "sgm_batch" else 0
    return (s.W, s.H, s.D, s.batch, s.paths, 0, vz, sampling, direction, adaptive, agg_mode)


def non_key(s):
    """what a call leaves in the plan without it being part of the key"""
    return (s.form, s.P1, s.P2, s.subpixel, s.vMax, s.d_min, s.vol_cmax, s.cost_bound, s.guide, s.want_S, s.want_C)


def plan_cmax(s):
    """the bound of the costs the plan selects its kernels for: 24 behind a cost stage, the volume's true maximum in the host
    forms of sgm(C), the declared bound in the device form"""
    if FAMILY[s.form] in ("calc_cost_sgm", "linear", "stereo"):
        return 24
    return s.cost_bound if s.form == "sgm_torch" else s.vol_cmax


def pipeline(s):
    """The name of the pipeline a fresh plan takes for this step.  Auto mode: the library's own fsgm_epi_auto_pipeline.  Mode 2
    (fused when eligible, the only forced mode the sequences draw) restates choose_pipeline: the block sweeps (8 paths) or the
    pair kernels (4) for D = 16 << k, 0 <= P1 <= P2, no wrap (cm + P2 + max(P1, P2) <= 255) and three / two y + P1 in a byte;
    the line kernels otherwise.  The GPU test holds every sgm step's reported kernel against this."""
    cm = plan_cmax(s)
    if s.agg_mode == 0 or FAMILY[s.form] != "sgm_batch":
        return epi.auto_pipeline(s.W, s.H, s.D, s.batch, s.paths, s.P1, s.P2, cm, adaptive_p2=key(s)[9])
    assert s.agg_mode == 2 and not s.adaptive
    if s.D not in LINE_D:
        return "generic"
    nowrap = cm + s.P2 + max(s.P1, s.P2) <= 255
    if s.D in FUSABLE_D and nowrap and s.P1 <= s.P2:
        if s.paths == 8 and 3 * (s.P1 + s.P2) <= 255:
            return "sweep16/nowrap"
        if s.paths == 4 and 2 * (s.P1 + s.P2) <= 255:
            return "pairs16/nowrap"
    return "packed16/nowrap" if nowrap else "packed16/wrap"


def pipeline_class(name):
    return "generic" if name == "generic" else "lines" if name.startswith("packed16") else "fused"


# ------------------------------------------------------------------------------------------------------------------ the draws
def _pick(r, seq):
    return seq[int(r.randint(len(seq)))]


# what each form takes and gives back beyond the penalties
_HAS = {"calc_cost_sgm": {"vMax", "subpixel", "S", "C"}, "calc_cost_sgm_mex": {"vMax"}, "calc_cost_sgm_linear": {"subpixel", "S", "C"},
        "stereo_sgm": {"d_min", "subpixel"}, "sgm": {"volume", "S"}, "sgm_batch": {"volume", "bound", "subpixel", "S"},
        "sgm_torch": {"volume", "bound", "subpixel", "S"}}


def _non_key(r, form):
    """the non-key half of a step, drawn for `form` (fields that the form does not have keep their neutral value)"""
    P1, P2 = _pick(r, PENALTIES)
    subpixel = int(r.rand() < 0.6)
    vMax = _pick(r, VMAX)
    d_min = _pick(r, D_MIN)
    vol_cmax = _pick(r, VOL_CMAX)
    cost_bound = _pick(r, COST_BOUND)
    want_S, want_C = bool(r.rand() < 0.4), bool(r.rand() < 0.3)
    guide = bool(r.rand() < 0.3)
    seed = int(r.randint(4))                                    # a small pool: inputs and expectations repeat
    has = _HAS[form]
    if "vMax" not in has:
        vMax = 0.3
    if "d_min" not in has:
        d_min = None
    if "volume" not in has:
        vol_cmax, cost_bound, guide = 24, 255, False
    if "bound" not in has:
        cost_bound, guide = 255, False
    if "subpixel" not in has:
        subpixel = 1
    if form == "sgm_batch":
        cost_bound = max(cost_bound, vol_cmax)                  # (a volume above the bound is a refusal: drawn on purpose only)
    want_S, want_C = want_S and "S" in has, want_C and "C" in has
    return dict(P1=P1, P2=P2, subpixel=subpixel, vMax=vMax, d_min=d_min, vol_cmax=vol_cmax, cost_bound=cost_bound, guide=guide,
                want_S=want_S, want_C=want_C, seed=seed)


def _step(r, form, W, H, D, batch, paths, vz=0, adaptive=0, agg_mode=0, direction=-1, **fixed):
    nk = _non_key(r, form)
    nk.update(fixed)
    if adaptive and FAMILY[form] == "sgm_batch":
        nk["guide"] = True
    return Step(form=form, W=W, H=H, D=D, batch=batch, paths=paths, vz=vz, adaptive=adaptive, agg_mode=agg_mode,
                direction=direction, refuse=None, **nk)


def _fresh(r):
    """a step of a random form on a random key"""
    form = _pick(r, ("calc_cost_sgm", "calc_cost_sgm_mex", "calc_cost_sgm_linear", "stereo_sgm", "sgm", "sgm_batch", "sgm_torch"))
    W, H, D = _pick(r, EPI_SHAPES)
    batch, paths = int(r.randint(1, 4)), int(_pick(r, (4, 8)))
    vz, adaptive, direction = int(r.rand() < 0.5), int(r.rand() < 0.3), int(_pick(r, (-1, 1)))
    if form == "calc_cost_sgm_mex":
        batch, paths, vz, adaptive = 1, 4, 1, 0
    if form == "sgm":
        batch, adaptive = 1, 0
    return _step(r, form, W, H, D, batch, paths, vz=vz, adaptive=adaptive, direction=direction)


def _again(r, s, forms=None):
    """another call on s's key: one of the forms that share it, the non-key half drawn anew"""
    form = _pick(r, forms or _SHARING[FAMILY[s.form]])
    return _step(r, form, s.W, s.H, s.D, s.batch, s.paths, vz=s.vz, adaptive=s.adaptive, agg_mode=s.agg_mode, direction=s.direction)


_SHARING = {"calc_cost_sgm": ("calc_cost_sgm",), "linear": ("calc_cost_sgm_linear",), "stereo": ("stereo_sgm",),
            "sgm": ("sgm",), "sgm_batch": ("sgm_batch", "sgm_torch")}


def _refusal(r, s):
    """a call the library refuses before it looks for a plan, on the shape of s"""
    kind = _pick(r, ("adaptive_p2 needs the guide image", "above cost_bound"))
    base = _step(r, "sgm_batch", s.W, s.H, s.D, s.batch, s.paths)
    if kind.startswith("adaptive"):
        return base._replace(adaptive=1, guide=False, refuse=kind)
    return base._replace(vol_cmax=255, cost_bound=24, refuse=kind)


def epi_sequence(seed, length=30):
    """test_epi_sequence: a list of Steps.
      1. a forced-mode key of sgm(C) walked through penalties, volumes and bounds by its host and device forms -- among them a pair
         of calls that differ in the bound of the costs alone, on either side of the no-wrap budget;
      2. one auto-mode key of a single frame visited by every family that shares it: sgm, sgm_batch, the device form, and
         calc_cost_sgm without the vz conversion;
      3. as many further keys as the cache holds, which evict both, and a return to each; then a rectified key through three
         search ranges (d_min -17, none, 7);
      4. free draws: a seen key again (six in ten), a new one, or a refusal (one in ten)."""
    r = rng(seed)
    steps = []
    # 1.
    W, H, D = _pick(r, [sh for sh in EPI_SHAPES if sh[2] in FUSABLE_D])
    batch, paths = int(r.randint(1, 4)), int(_pick(r, (4, 8)))
    inside = (21, 64) if paths == 8 else (63, 64)               # on the fused pipeline's byte budget
    k0 = _step(r, "sgm_torch", W, H, D, batch, paths, agg_mode=2, P1=inside[0], P2=inside[1], vol_cmax=24, cost_bound=127)
    steps.append(k0)
    steps.append(_again(r, k0, ("sgm_torch",))._replace(P1=inside[0], P2=inside[1], vol_cmax=24, cost_bound=255))    # the bound alone
    steps.append(_again(r, k0, ("sgm_batch",))._replace(P1=inside[0], P2=inside[1], vol_cmax=24, cost_bound=24))     # and back, host form
    steps.append(_again(r, k0, ("sgm_batch",))._replace(P1=inside[0], P2=inside[1], vol_cmax=255, cost_bound=255))   # the volume alone
    for _ in range(4):
        steps.append(_again(r, k0))
    # 2.
    W1, H1, D1 = _pick(r, EPI_SHAPES)
    paths1 = int(_pick(r, (4, 8)))
    k1 = _step(r, "sgm_torch", W1, H1, D1, 1, paths1, vol_cmax=24, cost_bound=24, P1=6, P2=64)
    steps.append(k1)
    order = ["sgm", "calc_cost_sgm", "sgm_batch", "sgm_torch", "sgm", "calc_cost_sgm"]
    r.shuffle(order)
    for form in order:
        steps.append(_step(r, form, W1, H1, D1, 1, paths1))
    # 3.
    seen = {key(s) for s in steps}
    fresh = []
    while len(fresh) < EPI_CAP:
        s = _fresh(r)
        if not fresh:                                           # the first of them through the MEX gateway, as shipped
            s = _step(r, "calc_cost_sgm_mex", s.W, s.H, s.D, 1, 4, vz=1)
        if key(s) not in seen:
            seen.add(key(s))
            fresh.append(s)
    steps += fresh
    steps.append(_again(r, k0))
    steps.append(_again(r, k1, ("sgm", "sgm_batch", "sgm_torch")))
    # (a rectified key through three search ranges: the shift is no part of the key)
    Ws, Hs, Ds = _pick(r, EPI_SHAPES)
    ks = _step(r, "stereo_sgm", Ws, Hs, Ds, int(r.randint(1, 4)), int(_pick(r, (4, 8))), direction=int(_pick(r, (-1, 1))), d_min=-17)
    steps += [ks, _again(r, ks)._replace(d_min=None), _again(r, ks)._replace(d_min=7)]
    # 4.
    while len(steps) < length:
        u = r.rand()
        if u < 0.1:
            steps.append(_refusal(r, _pick(r, steps)))
        elif u < 0.7:
            steps.append(_again(r, _pick(r, [s for s in steps if s.refuse is None])))
        else:
            steps.append(_fresh(r))
    return steps


EPI_SEEDS = tuple(range(8))


# ------------------------------------------------------------------------------------------------------- the cache, restated
def cache_walk(steps, cap=EPI_CAP):
    """What PlanCache does with the steps' keys: first in, first out at the cap, a hit moves nothing.  Per step a dict:
    hit (the key was resident), prev (index of the last call on this key since it was last created, or None), returned (the key
    had been evicted before and is created again), evicted (the key this step pushed out, or None).  A refused step never reaches
    the cache."""
    resident, last, gone, out = [], {}, set(), []
    for i, s in enumerate(steps):
        if s.refuse is not None:
            out.append(dict(hit=False, prev=None, returned=False, evicted=None))
            continue
        k = key(s)
        hit = k in resident
        evicted = None
        if not hit:
            if len(resident) >= cap:
                evicted = resident.pop(0)
                gone.add(evicted)
                last.pop(evicted, None)
            resident.append(k)
        out.append(dict(hit=hit, prev=last.get(k), returned=(not hit and k in gone), evicted=evicted))
        last[k] = i
    return out


# ------------------------------------------------------------------------------------------------- inputs and expectations
def _edge(I1):
    """a step edge down the middle: adaptive P2 matters (tests/test_gpu_sgm_device.py)"""
    I1 = I1.copy()
    W = I1.shape[1]
    I1[:, W // 2:] = np.minimum(I1[:, W // 2:].astype(np.int32) + 120, 255).astype(np.uint8)
    return I1


@functools.lru_cache(maxsize=None)
def images(W, H, D, seed, f):
    I1, I2 = synth.image_pair(W, H, D, seed=100 + 10 * seed + f)
    I1 = _edge(I1)
    for a in (I1, I2):
        a.setflags(write=False)
    return I1, I2


@functools.lru_cache(maxsize=None)
def maps(W, H, seed):
    m = synth.epi_maps(W, H, "general", seed=5 + seed)
    for a in m:
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def volume(W, H, D, cmax, seed, f):
    v = BV.volume(("uniform", "columns", "minimum")[(seed + f) % 3], W, H, D, cmax, 300 + 10 * seed + f)
    assert int(v.max()) == cmax
    v.setflags(write=False)
    return v


def volumes(s):
    return np.stack([volume(s.W, s.H, s.D, s.vol_cmax, s.seed, f) for f in range(s.batch)])


def guides(s):
    return np.stack([images(s.W, s.H, s.D, s.seed, f)[0] for f in range(s.batch)])


@functools.lru_cache(maxsize=None)
def _cost(form, W, H, D, seed, f, vMax, direction, d_min):
    from oracle import pyoracle
    from tests import stereo_restatement as SR, stereo_range_restatement as RR
    I1, I2 = images(W, H, D, seed, f)
    if form == "vz":
        return pyoracle.epi_cost(I1, I2, D, vMax, *maps(W, H, seed))
    if form == "linear":
        pd0, nd, _ = maps(W, H, seed)
        return SR.linear_cost(I1, I2, D, pd0, nd)
    pd0, nd = RR.shifted_maps(W, H, direction, d_min)
    return SR.linear_cost(I1, I2, D, pd0, nd)


@functools.lru_cache(maxsize=None)
def _aggregate(vol_key, P1, P2, paths, adaptive):
    """S (flat, one word past the end) of a volume named by the arguments that make it; adaptive: with the frame's first image"""
    from oracle import pyoracle
    from tests import adaptive_p2_restatement as A
    Cv, I1 = _VOLUMES[vol_key]
    return A.aggregate(Cv, I1, P1, P2, paths, 1) if adaptive else pyoracle.epi_aggregate(Cv, P1, P2, paths)


_VOLUMES = {}


def expected(s):
    """dict of the arrays the step must return, frames stacked: bestD, minC, and S / C where asked for; status for the device
    form.  From the oracle and the restatements (adaptive_p2_restatement, stereo_restatement, stereo_range_restatement)."""
    from oracle import pyoracle
    from tests import stereo_range_restatement as RR
    fam = FAMILY[s.form]
    out = collections.defaultdict(list)
    for f in range(s.batch):
        I1 = images(s.W, s.H, s.D, s.seed, f)[0]
        if fam in ("sgm", "sgm_batch"):
            vk = ("vol", s.W, s.H, s.D, s.vol_cmax, s.seed, f, s.cost_bound if s.form == "sgm_torch" else 255)
            if vk not in _VOLUMES:
                _VOLUMES[vk] = (np.minimum(volume(s.W, s.H, s.D, s.vol_cmax, s.seed, f), vk[-1]), I1)
        else:
            form = {"calc_cost_sgm": "vz", "linear": "linear", "stereo": "rect"}[fam]
            args = (form, s.W, s.H, s.D, s.seed, f, s.vMax if form == "vz" else 0.0, s.direction if form == "rect" else 0,
                    (s.d_min or 0) if form == "rect" else 0)
            vk = ("cost",) + args
            if vk not in _VOLUMES:
                _VOLUMES[vk] = (_cost(*args), I1)
        S = _aggregate(vk, s.P1, s.P2, s.paths, key(s)[9])
        bestD, minC = pyoracle.epi_wta(S, s.W, s.H, s.D, s.subpixel)
        if fam == "calc_cost_sgm" and s.vz:
            bestD = pyoracle.epi_vz_to_disp(bestD, maps(s.W, s.H, s.seed)[2], s.vMax, s.D + 1)
        if fam == "stereo" and s.d_min is not None:
            bestD = RR.true_disp(bestD, s.d_min)
        out["bestD"].append(bestD)
        out["minC"].append(minC)
        if s.want_S:
            out["S"].append(np.asarray(S)[:-1].reshape(s.H, s.W, s.D))
        if s.want_C:
            out["C"].append(_VOLUMES[vk][0])
    res = {k: np.stack(v) for k, v in out.items()}
    if s.form == "sgm_torch":
        res["status"] = 1 if s.vol_cmax > s.cost_bound else 0
    return res


# ------------------------------------------------------------------------------------------------------------- the calls
def run(s, host_only=False, stream=None):
    """The step's call; returns a dict like expected()'s.  host_only (no device at hand: the argument checks alone): the device
    form goes through fsgm_sgm_batch_host, which shares its check table, with the volume saturated as the device would.
    stream: the torch stream the device form is queued on (synchronised before the outputs are read)."""
    import fsgm_amd
    from fsgm_amd.sgm import sgm_batch
    fam = FAMILY[s.form]
    B = s.batch
    frames = [images(s.W, s.H, s.D, s.seed, f) for f in range(B)]
    out = {}
    if fam in ("calc_cost_sgm", "linear"):
        pd0, nd, off = maps(s.W, s.H, s.seed)
        if s.form == "calc_cost_sgm_mex":
            from tests import mexharness as mh
            (bd, mc), _ = mh.call("calc_cost_sgm", 2, frames[0][0], frames[0][1], s.D, s.vMax, pd0, nd, off, s.P1, s.P2)
            return dict(bestD=bd[None], minC=mc[None])
        vol = s.want_S or s.want_C
        if fam == "linear":
            res = fsgm_amd.epi.calc_cost_sgm_linear_batch([(a, b, pd0, nd) for a, b in frames], s.D, s.P1, s.P2, paths=s.paths,
                                                          subpixel=s.subpixel, return_volumes=vol, adaptive_p2=s.adaptive)
        else:
            res = fsgm_amd.calc_cost_sgm_batch([(a, b, pd0, nd, off) for a, b in frames], s.D, s.vMax, s.P1, s.P2, paths=s.paths,
                                               subpixel=s.subpixel, vz_to_disp=s.vz, return_volumes=vol, adaptive_p2=s.adaptive)
        out["bestD"], out["minC"] = (np.stack([r[k] for r in res]) for k in (0, 1))
        if s.want_C:
            out["C"] = np.stack([r[2] for r in res])
        if s.want_S:
            out["S"] = np.stack([r[3] for r in res])
        return out
    if fam == "stereo":
        left, right = (np.stack([fr[k] for fr in frames]) for k in (0, 1))
        out["bestD"], out["minC"] = fsgm_amd.stereo_sgm(left, right, s.D, s.P1, s.P2, paths=s.paths, subpixel=s.subpixel,
                                                        direction=s.direction, adaptive_p2=s.adaptive, d_min=s.d_min)
        return out
    vols = volumes(s)
    guide = guides(s) if s.guide else None
    if s.form == "sgm":
        res = fsgm_amd.sgm(vols[0], s.P1, s.P2, paths=s.paths, return_sum=s.want_S)
        res = tuple(a[None] for a in res)
    elif s.form == "sgm_batch" or host_only:
        if s.form == "sgm_torch":
            vols = np.minimum(vols, s.cost_bound)
        res = sgm_batch(vols, s.P1, s.P2, paths=s.paths, cost_bound=s.cost_bound, agg_mode=s.agg_mode, adaptive_p2=s.adaptive,
                        guide=guide, subpixel=s.subpixel, return_sum=s.want_S)
    else:
        import torch
        from fsgm_amd import torch_ops
        with torch.cuda.stream(stream):
            Ct = torch.from_numpy(np.ascontiguousarray(vols.transpose(0, 3, 1, 2))).to("cuda:0", non_blocking=True)
            gt = None if guide is None else torch.from_numpy(guide).to("cuda:0", non_blocking=True)
            res = torch_ops.sgm(Ct, s.P1, s.P2, layout="dhw", paths=s.paths, cost_bound=s.cost_bound, agg_mode=s.agg_mode,
                                adaptive_p2=s.adaptive, guide=gt, subpixel=s.subpixel, return_sum=s.want_S, return_status=True)
        stream.synchronize()
        out["status"] = int(res[-1].item())
        res = tuple(t.cpu().numpy() for t in res[:-1])
    out["bestD"], out["minC"] = res[0], res[1]
    if s.want_S:
        out["S"] = res[2]
    return out


# =====================================================================================================================
# The other caches: g_pyd and g_sgm2d (cap 6), the neighbour-guided arena, the two pyramid caches (cap 2), g_post / g_flow /
# g_spp (cap 4).  A step names its cache, the form of the call (Python wrapper, MEX gateway, torch op on a side stream, ...),
# the key the cache finds the plan by, the parameters that are no part of it, and the seed of its data.
OStep = collections.namedtuple("OStep", ["cache", "form", "key", "nk", "seed"])
GROUPS = ("pyd_sgm2d", "ng", "pyramids", "post")
OTHER_SEEDS = (0, 1, 2, 3)
CAPS = {"pyd": 6, "sgm2d": 6, "ng": None, "pyramid": 2, "ng_pyramid": 2, "post": 4, "flow": 4, "spp": 4}
CACHES = {"pyd_sgm2d": ("pyd", "sgm2d"), "ng": ("ng",), "pyramids": ("pyramid", "ng_pyramid"), "post": ("post", "flow", "spp")}
FORMS = {"pyd": ("py", "mex"), "sgm2d": ("host", "torch"), "ng": ("py", "batch", "mex"), "pyramid": ("host", "torch"),
         "ng_pyramid": ("host", "torch"), "post": ("host", "torch"), "flow": ("host", "torch"), "spp": ("host", "torch")}
SMALL = [(21, 13), (29, 17), (17, 11), (13, 12)]
# keys.  pyd: (W, H, rX, rY, rAgg); sgm2d: (W, H, rX, rY, frames, adaptive: the plan holds a guide) with windows that never take
# the row-packed kernels (a side above 11), so the reported aggregation follows from the bound alone; ng: none -- one arena;
# pyramids: (W, H, numPyd, P2), every parameter is part of the key; post / flow / spp: (W, H, frames)
KEYS = {
    "pyd": [(W, H, rX, rY, 2) for W, H in SMALL[:3] for rX, rY in ((2, 1), (1, 2), (3, 3))],
    "sgm2d": [(W, H, rX, rY, n, a) for W, H in SMALL[:2] for rX, rY in ((6, 1), (1, 6)) for n in (1, 2) for a in (0, 1)],
    "ng": [()],
    "pyramid": [(W, H, n, P2) for W, H in ((41, 29), (37, 23)) for n in (2, 3) for P2 in (32, 40)],
    "ng_pyramid": [(W, H, n, P2) for W, H in ((41, 29), (37, 23)) for n in (2, 3) for P2 in (32, 64)],
    "post": [(W, 7, n) for W in range(11, 15) for n in (1, 2)],
    "flow": [(W, 7, n) for W in range(11, 15) for n in (1, 2)],
    "spp": [(W, 7, n) for W in range(11, 15) for n in (1, 2)],
}


def _other_nk(r, cache):
    """the non-key half, drawn for `cache`"""
    if cache == "pyd":       # (subPixelRefine, P1, P2, diagonal, totalPass, adaptiveP2)
        return (int(r.rand() < 0.5),) + _pick(r, [(6, 32), (100, 200), (0, 0)]) + (int(r.rand() < 0.6), int(_pick(r, (1, 2, 3))), int(r.rand() < 0.5))
    if cache == "sgm2d":     # (P1, P2, diagonal, totalPass, subpixel, hints, cmax = bound)
        return _pick(r, [(6, 32), (100, 200)]) + (int(r.rand() < 0.6), int(_pick(r, (1, 2))), int(r.rand() < 0.5), bool(r.rand() < 0.5),
                                                   int(_pick(r, (24, 255))))
    if cache == "ng":        # (W, H, halfSearchWinSize, aggSize, subPixelRefine, P1, P2, frames, S asked for)
        return _pick(r, [(16, 12), (8, 6), (24, 18)]) + (int(_pick(r, (0, 1, 2))), int(_pick(r, (2, 3))), int(r.rand() < 0.5)) + \
            _pick(r, [(6, 32), (20, 64)]) + (int(_pick(r, (1, 1, 2, 3))), bool(r.rand() < 0.4))
    if cache in ("pyramid", "ng_pyramid"):
        return ()
    if cache == "post":      # (vMax, dMax)
        return (_pick(r, (0.3, 0.5)), int(_pick(r, (64, 32))))
    if cache == "flow":      # (stage, its threshold)
        return _pick(r, [("speckle", 4.0), ("speckle", 100.0), ("fb", 2.0), ("fb", 0.5), ("fill", 0.0)])
    return (_pick(r, ("fb", "second")), int(_pick(r, (0, -3, 5))), int(_pick(r, (-1, 1))), _pick(r, (1.0, 2.0)))    # spp


def _other_form(r, cache, nk):
    form = _pick(r, FORMS[cache])
    if cache == "flow" and nk[0] != "fb" or cache == "spp" and nk[0] != "fb":
        form = "host"                                           # (the torch ops offer the checks)
    if cache == "ng":
        form = "batch" if nk[7] > 1 else _pick(r, ("py", "mex"))
        if form == "mex":
            nk = nk[:8] + (False,)                              # (the gateway returns no S)
    return form, nk


def _other_step(r, cache, k):
    nk = _other_nk(r, cache)
    form, nk = _other_form(r, cache, nk)
    return OStep(cache, form, k, nk, int(r.randint(3)))


def other_sequence(group, seed, length=None):
    """test_other_sequence: per cache of the group four calls on one key (other parameters, other forms), then as many other
    keys as the cache holds and the first key again; free draws -- a seen key again, six in ten -- fill the rest.  The arena
    of the neighbour-guided level has no key: its steps walk sizes, batches and search windows."""
    r = np.random.RandomState(9000 + 100 * GROUPS.index(group) + seed)
    steps, first = [], {}
    for cache in CACHES[group]:
        keys = list(KEYS[cache])
        r.shuffle(keys)
        first[cache] = keys
        steps += [_other_step(r, cache, keys[0]) for _ in range(4)]
    for cache in CACHES[group]:
        cap, keys = CAPS[cache], first[cache]
        if cap is None:
            continue
        steps += [_other_step(r, cache, k) for k in keys[1:cap + 1]] + [_other_step(r, cache, keys[0])]
    length = length or {"pyd_sgm2d": 28, "ng": 14, "pyramids": 18, "post": 32}[group]
    while len(steps) < length:
        cache = _pick(r, CACHES[group])
        seen = [s.key for s in steps if s.cache == cache]
        steps.append(_other_step(r, cache, _pick(r, seen) if r.rand() < 0.6 else _pick(r, KEYS[cache])))
    return steps


def other_walk(steps):
    """cache_walk for steps of several caches: each cache first in, first out at its own cap (the arena: always resident)"""
    resident, last, gone, out = collections.defaultdict(list), {}, set(), []
    for i, s in enumerate(steps):
        k, cap = (s.cache, s.key), CAPS[s.cache]
        hit = k in resident[s.cache]
        evicted = None
        if not hit:
            if cap is not None and len(resident[s.cache]) >= cap:
                evicted = resident[s.cache].pop(0)
                gone.add(evicted)
                last.pop(evicted, None)
            resident[s.cache].append(k)
        out.append(dict(hit=hit, prev=last.get(k), returned=(not hit and k in gone), evicted=evicted))
        last[k] = i
    return out


def ng_need(s):
    """bytes of candidate buffers an ng step asks of the arena (ng_level_bufs: 24 bytes a candidate)"""
    W, H, half, _, _, _, _, frames, _ = s.nk
    return W * H * 9 * (2 * half + 1) ** 2 * frames * 24


def sgm2d_want(oracle, vols, hints, guide, rX, rY, P1, P2, bound, diag, passes, adaptive, sub):
    """(bestD, minC, mvSub, flow, S) per frame: pyd_wta(pyd_aggregate(guide, min(C, bound), hints or zeros)) (tests/test_gpu_sgm2d.py)"""
    n, H, W, _ = vols.shape
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    out = []
    for f in range(n):
        mv = np.zeros((2, H, W)) if hints is None else hints[f]
        S = oracle.pyd_aggregate(guide[f], np.minimum(vols[f], bound), mv, Sx, Sy, P1, P2, diag, passes, adaptive)
        bd, mc, ms = oracle.pyd_wta(S, Sx, Sy, sub)
        off = np.stack([bd // Sy, bd % Sy]).astype(np.float64) - np.array([rX, rY], np.float64)[:, None, None]
        out.append((bd, mc, ms, mv[:, :H, :W] + off + ms, S))
    return tuple(np.stack([o[k] for o in out]) for k in range(5))


def sgm2d_inputs(W, H, rX, rY, n, seed, cmax):
    D = (2 * rX + 1) * (2 * rY + 1)
    vols = np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)])
    hints = np.stack([synth.hint_map(W, H, "general", seed=seed + 5 * f, amp=3.0) for f in range(n)])      # of the image's size:
    guide = np.stack([synth.image_pair(W, H, 16, seed=seed + f)[0] // 2 for f in range(n)])               # one key with or without
    guide[:, :, W // 2:] += 120
    return vols, hints, guide




# ------------------------------------------------------------------------------------- the other caches: calls and expectations
def _pair(W, H, seed):
    return synth.image_pair(W, H, 16, seed=40 + 7 * seed + W)


@functools.lru_cache(maxsize=None)
def other_inputs(s):
    """the arrays the step's call takes (a tuple, by cache), from its key, its seed and -- the arena's steps -- its parameters"""
    from tests import flow_pp_inputs, stereo_pp_restatement as SP
    if s.cache == "pyd":
        W, H = s.key[:2]
        return _pair(W, H, s.seed) + (synth.hint_map(W, H, "general", seed=60 + s.seed, amp=3.0),)
    if s.cache == "sgm2d":
        W, H, rX, rY, n, _ = s.key
        return sgm2d_inputs(W, H, rX, rY, n, 3 + s.seed, s.nk[6])
    if s.cache in ("pyramid", "ng_pyramid"):
        return _pair(s.key[0], s.key[1], s.seed)
    W, H, n = s.key
    if s.cache == "post":
        g = [synth.epi_maps(W, H, ("general", "radial")[f % 2], seed=W + 10 * s.seed + f) for f in range(n)]
        D1 = np.stack([synth.vz_index_map(W, H, s.nk[1], seed=W + s.seed + f, invalid=0.1) for f in range(n)])
        return (D1, np.stack([x[0] for x in g]), np.stack([x[1] for x in g]), np.stack([x[2] / 8 for x in g]))
    if s.cache == "flow":
        fb = [flow_pp_inputs.flow_pair(W, H, ("general", "int")[f % 2], seed=W + s.seed + f) for f in range(n)]
        return (np.stack([x[0] for x in fb]), np.stack([x[1] for x in fb]))
    return (np.stack([SP.stage_maps(W, H, 24, seed=5 + s.seed + f)["random"] for f in range(n)]),)      # spp


def _ng_frames(s):
    from oracle import pyoracle
    from tests import ng_helpers as NG
    W, H, half, agg, sub, P1, P2, frames, _ = s.nk
    return NG.ng_frames(pyoracle, W, H, frames, "general", 2.0, r=half, sub=sub, agg=agg, P1=P1, P2=P2)


@functools.lru_cache(maxsize=None)
def other_expected(s):
    """the tuple of arrays the step must return, from the oracle and the restatements alone"""
    from oracle import pyoracle
    from tests import flow_pp_restatement as FR, stereo_pp_restatement as SP
    from tests.edge_inputs import oracle_pyramidal_ng
    inp = () if s.cache == "ng" else other_inputs(s)
    if s.cache == "pyd":
        _, _, rX, rY, rAgg = s.key
        return pyoracle.calc_pyd_cost_sgm(*inp, rX, rY, rAgg, *s.nk)
    if s.cache == "sgm2d":
        _, _, rX, rY, _, adaptive = s.key
        P1, P2, diag, passes, sub, hints, cmax = s.nk
        return sgm2d_want(pyoracle, inp[0], inp[1] if hints else None, inp[2], rX, rY, P1, P2, cmax, diag, passes, adaptive, sub)
    if s.cache == "ng":
        want = _ng_frames(s)[1]
        return tuple(np.stack([w[k] for w in want]) for k in ((0, 1, 3) if s.nk[8] else (0, 1)))
    if s.cache == "pyramid":
        return pyoracle.pyramidal_sgm(*inp, s.key[2], 6, s.key[3])[:2]
    if s.cache == "ng_pyramid":
        flows, mc = oracle_pyramidal_ng(pyoracle, *inp, s.key[2], 1, 2, 0, 6, s.key[3])
        return flows[-1], mc
    n = s.key[2]
    if s.cache == "post":
        vMax, dMax = s.nk
        per = [pyoracle.postprocess(inp[0][f], inp[1][f], inp[2][f], inp[3][f], vMax, dMax + 1, dMax) for f in range(n)]
        return tuple(np.stack([p[k] for p in per]) for k in range(3))
    if s.cache == "flow":
        op, thr = s.nk
        f, b = inp
        one = {"speckle": lambda k: FR.flow_speckle_filter(f[k], 2.0, thr)[0], "fb": lambda k: FR.flow_fb_check(f[k], b[k], thr)[0],
               "fill": lambda k: FR.flow_in_fill(f[k])}[op]
        return (np.stack([one(k) for k in range(n)]),)
    op, d_min, direction, thr = s.nk                            # spp
    second = [SP.stereo_disp_from_first(w, d_min, direction) for w in inp[0]]
    if op == "second":
        return (np.stack(second),)
    return (np.stack([SP.stereo_fb_check(w, d2, d_min, direction, thr) for w, d2 in zip(inp[0], second)]),)


def other_run(s, host_only=False, stream=None):
    """the step's call; a tuple like other_expected's.  host_only: the torch forms through the host entry of the same cache.
    stream: the torch stream the device forms are queued on."""
    import fsgm_amd
    from tests import mexharness as mh
    inp = () if s.cache == "ng" else other_inputs(s)
    dev = s.form == "torch" and not host_only
    if dev:
        import torch
        from fsgm_amd import torch_ops

        def on_stream(call):
            with torch.cuda.stream(stream):
                t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", non_blocking=True)  # noqa: E731
                res = call(t)
            stream.synchronize()
            return tuple(x.cpu().numpy() for x in (res if isinstance(res, tuple) else (res,)))
    if s.cache == "pyd":
        _, _, rX, rY, rAgg = s.key
        if s.form == "mex":
            return tuple(mh.call("calc_pyd_cost_sgm", 3, *inp, rX, rY, rAgg, *s.nk)[0])
        return fsgm_amd.calc_pyd_cost_sgm(*inp, rX, rY, rAgg, *s.nk)
    if s.cache == "sgm2d":
        _, _, rX, rY, _, adaptive = s.key
        P1, P2, diag, passes, sub, hints, cmax = s.nk
        vols, hm, guide = inp
        src = np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
        kw = dict(layout="dhw", cost_bound=cmax, diagonal=diag, total_pass=passes, adaptive_p2=adaptive, subpixel=sub, return_flow=True,
                  return_sum=True)
        hm, guide = (hm if hints else None), (guide if adaptive else None)
        if dev:
            return on_stream(lambda t: torch_ops.sgm2d(t(src), rX, rY, P1, P2, hints=t(hm), guide=t(guide), **kw))
        return fsgm_amd.sgm2d_batch(src, rX, rY, P1, P2, hints=hm, guide=guide, **kw)
    if s.cache == "ng":
        _, _, half, agg, sub, P1, P2, frames, want_S = s.nk
        fr = _ng_frames(s)[0]
        if s.form == "mex":
            return tuple(a[None] for a in mh.call("calc_pyd_cost_sgm_ng", 2, *fr[0], half, agg, sub, P1, P2)[0])
        if s.form == "batch":
            res = fsgm_amd.calc_pyd_cost_sgm_ng_batch(fr, half, agg, sub, P1, P2)
            out = tuple(np.stack([x[k] for x in res]) for k in (0, 1))
            return out + (other_expected(s)[2],) if want_S else out         # (the batch form returns no S)
        return tuple(a[None] for a in fsgm_amd.calc_pyd_cost_sgm_ng(*fr[0], half, agg, sub, P1, P2, return_sum=want_S))
    if s.cache in ("pyramid", "ng_pyramid"):
        host, op = ((fsgm_amd.pyramidal_sgm, "pyramidal_sgm") if s.cache == "pyramid" else (fsgm_amd.pyramidal_sgm_ng, "pyramidal_sgm_ng"))
        if dev:
            return on_stream(lambda t: getattr(torch_ops, op)(t(inp[0]), t(inp[1]), s.key[2], P2=s.key[3]))
        mv, _, mc = host(*inp, s.key[2], P2=s.key[3])
        return mv, mc
    if s.cache == "post":
        vMax, dMax = s.nk
        if dev:
            return on_stream(lambda t: torch_ops.epi_postprocess(*[t(a) for a in inp], vMax, dMax + 1, dMax))
        return tuple(fsgm_amd.epi_postprocess_batch(*inp, vMax, dMax + 1, dMax))
    if s.cache == "flow":
        op, thr = s.nk
        if dev:
            return on_stream(lambda t: torch_ops.flow_fb_check(t(inp[0]), t(inp[1]), thr))
        return ({"speckle": lambda: fsgm_amd.flow_speckle_filter(inp[0], 2, thr), "fb": lambda: fsgm_amd.flow_fb_check(inp[0], inp[1], thr),
                 "fill": lambda: fsgm_amd.flow_in_fill(inp[0])}[op](),)
    op, d_min, direction, thr = s.nk                            # spp
    if dev:
        return on_stream(lambda t: torch_ops.stereo_fb_check(t(inp[0]), None, d_min, direction, thr))
    if op == "second":
        return (fsgm_amd.stereo_disp_from_first(inp[0], d_min, direction),)
    return (fsgm_amd.stereo_fb_check(inp[0], None, d_min, direction, thr),)


def sgm2d_kernel(s):
    """fsgm_sgm2d_last_kernel of a fresh plan: these windows never take the row-packed kernels, the bound decides the rest"""
    P1, P2, cmax = s.nk[0], s.nk[1], s.nk[6]
    return "generic/wrap" if cmax + P2 + max(P1, P2) > 255 else "generic"
