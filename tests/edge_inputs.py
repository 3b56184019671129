"""Edge-value input generators for the sweeps of the post-processing chain, vmf, the pyramidal drivers and the epipolar maps
(tests/test_gpu_edge_sweeps.py, tests/test_oracle_edge_cpu.py), and the oracle compositions those sweeps compare against.

Every generator takes a numpy RandomState and draws shapes, parameters and data that sit where order-free restatements of
raster-order code go wrong: ties on the comparison thresholds, regions one pixel either side of the size threshold, +-0.0,
+Inf, subnormals, huge values, NaN rows / columns / frames, targets on the image border and on round-half points."""
import numpy as np

from fsgm_amd import synth

NAN, INF = np.nan, np.inf
TINY = (5e-324, 2.2250738585072014e-308 / 3, 2.2250738585072014e-308)           # subnormals, the smallest normal
HUGE = (1e300, 1.7976931348623157e308, 2.0 ** 53 + 1.0, 2.0 ** 52 + 1.0)


def rng(seed):
    return np.random.RandomState(seed)


def pred(x):
    return np.nextafter(x, -np.inf)


def pick_size(r, lo, hi, edges):
    """A size in lo..hi, two times in three one of the listed edge sizes."""
    edges = [e for e in edges if lo <= e <= hi]
    return int(r.choice(edges)) if edges and r.rand() < 0.67 else int(r.randint(lo, hi + 1))


POST_EDGES = (1, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def post_shape(r, small=False):
    """(W, H, N): tile edges (64x4), the 256-column chunks of the row scans and the 1024-pixel chunks of the label ranks.  One side
    long at most, so that a frame stays below ~40k pixels (the oracle's time)."""
    hi = 40 if small else 300
    W = pick_size(r, 1, 513 if not small else hi, POST_EDGES)
    H = pick_size(r, 1, max(1, min(hi, 40000 // W)), POST_EDGES)
    return W, H, int(r.randint(1, 4 if small else 10))


def post_params(r):
    """(maxDiff, maxSize, vMax, n, dMax) on the 1/256 grid of the maps, maxSize 0 and 1 and maxDiff 0 included.  vMax * 2 is
    exact, so w = n / vMax makes vzRatio exactly 1."""
    maxDiff = float(r.choice([0.0, 1 / 256, 2 / 256, 0.5, 1.0, 2.0, 3.0, 64.0]))
    maxSize = float(r.choice([0, 1, 2, 3, 5, 8, 13, 100]))
    vMax = float(r.choice([0.25, 0.3, 0.5, 0.125]))
    dMax = int(r.choice([16, 32, 64, 20]))
    n = float(dMax + 1) if r.rand() < 0.7 else float(r.choice([1, 8, 65]))
    if r.rand() < 0.15:
        dMax = float(r.choice([0.0, 1 / 256, 2.0]))
    return maxDiff, maxSize, vMax, n, dMax


def _plant_region(r, m, k, value):
    """k pixels (the first k of a rectangle in raster order: 4-connected) of one value, cut off by a ring of NaN."""
    H, W = m.shape
    if k <= 0:
        return
    w = int(min(W, max(1, r.randint(1, 12)), k))
    h = -(-k // w)
    if h > H:
        return
    y0, x0 = int(r.randint(0, H - h + 1)), int(r.randint(0, W - w + 1))
    ya, yb, xa, xb = max(y0 - 1, 0), min(y0 + h + 1, H), max(x0 - 1, 0), min(x0 + w + 1, W)
    m[ya:yb, xa:xb] = NAN
    blk = np.full(h * w, NAN)
    blk[:k] = value
    m[y0:y0 + h, x0:x0 + w] = blk.reshape(h, w)


def post_maps(r, W, H, N, maxSize, vMax, n):
    """N non-negative vz maps (N, H, W): values on a 1/256 grid with small steps between neighbours (ties with maxDiff), regions
    of maxSize - 1, maxSize and maxSize + 1 pixels, +-0.0 (whole patches of -0.0 too), +Inf, subnormals, huge values, w = n / vMax,
    all-NaN rows in the middle, all-NaN columns, an all-NaN frame and a NaN-free frame."""
    D1 = np.empty((N, H, W))
    for f in range(N):
        step = float(r.choice([1 / 256, 2 / 256, 0.5, 1.0, 2.0]))
        base = float(r.randint(0, 40 * 256)) / 256
        m = base + np.cumsum(r.randint(-2, 3, (H, W)), axis=1) * step
        m = np.abs(m + r.randint(-1, 2, (H, 1)) * step)
        m[r.rand(H, W) < float(r.choice([0.0, 0.05, 0.3, 0.8]))] = NAN
        if f == N - 1 and N > 1 and r.rand() < 0.5:                 # a NaN-free frame: nothing planted either
            D1[f] = np.nan_to_num(m, nan=1.0)
            continue
        for k in (maxSize - 1, maxSize, maxSize + 1):
            if r.rand() < 0.8:
                _plant_region(r, m, int(k), float(r.choice([base + 100.0, 0.0, -0.0, 5.5])))
        flat = m.reshape(-1)
        specials = [0.0, -0.0, INF, n / vMax, *TINY, *HUGE, 0.5, 255 / 256]
        cnt = int(r.randint(0, max(2, W * H // 8)))
        flat[r.randint(0, W * H, cnt)] = r.choice(specials, cnt)
        if r.rand() < 0.4:                                          # a patch of -0.0
            y0, x0 = r.randint(0, H), r.randint(0, W)
            m[y0:y0 + int(r.randint(1, 6)), x0:x0 + int(r.randint(1, 9))] = -0.0
        if H >= 3 and r.rand() < 0.5:                               # all-NaN rows between valid rows
            m[r.randint(1, H - 1, int(r.randint(1, 3)))] = NAN
        if W >= 2 and r.rand() < 0.4:
            m[:, r.randint(0, W, int(r.randint(1, 3)))] = NAN
        D1[f] = m
    if N >= 3 and r.rand() < 0.5:
        D1[int(r.randint(0, N))] = NAN
    return D1


def post_geometry(r, W, H, N):
    """Pd0, nd (N, 2, H, W) and O (N, H, W).  Around an identity flow (so that forward-backward checks pass for some pixels), with
    pixels whose target is set exactly: nd = 0 (or O = 0) makes the target Pd0 itself, which is then 1, W, W + 1, 0, -1, k + 0.5,
    pred(k + 0.5) or -(k + 0.5); whole blocks aimed at one cell (contention on the maximum); NaN and +-Inf entries."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Pd0 = np.empty((N, 2, H, W))
    nd = np.empty((N, 2, H, W))
    O = np.empty((N, H, W))
    for f in range(N):
        jit = np.round((r.rand(2, H, W) - 0.5) * 8) / 8
        Pd0[f] = np.stack([xx + 1.0, yy + 1.0]) + jit
        ang = r.rand(H, W) * 2 * np.pi
        nd[f] = np.stack([np.cos(ang), np.sin(ang)])
        O[f] = float(r.choice([0.0, 1 / 8, 1.0, 4.0])) * r.rand(H, W)
        for c, L in ((0, W), (1, H)):                               # exact targets
            k = r.randint(0, L + 1, (H, W)).astype(np.float64)
            exact = np.choose(r.randint(0, 8, (H, W)), [np.ones((H, W)), np.full((H, W), float(L)), np.full((H, W), L + 1.0),
                                                         np.zeros((H, W)), -np.ones((H, W)), k + 0.5, pred(k + 0.5), -(k + 0.5)])
            sel = r.rand(H, W) < 0.3
            Pd0[f, c][sel] = exact[sel]
            nd[f, c][sel] = 0.0
        if r.rand() < 0.5:                                          # a block aimed at one cell
            y0, x0 = r.randint(0, H), r.randint(0, W)
            ys, xs = slice(y0, y0 + int(r.randint(1, 9))), slice(x0, x0 + int(r.randint(1, 17)))
            Pd0[f, 0, ys, xs] = float(r.randint(1, W + 1)) + float(r.choice([0.0, 0.25]))
            Pd0[f, 1, ys, xs] = float(r.randint(1, H + 1))
            nd[f, :, ys, xs] = 0.0
        for a in (Pd0[f].reshape(-1), nd[f].reshape(-1), O[f].reshape(-1)):
            cnt = int(r.randint(0, 3))
            a[r.randint(0, a.size, cnt)] = r.choice([NAN, INF, -INF], cnt)
    return Pd0, nd, O


def vmf_flows(r, W, H, N, ch):
    """(N, ch, H, W) flows: values on a coarse grid (ties), +-0.0, +-Inf, huge values, NaN pixels, rows, columns and blocks, and
    NaN-free frames."""
    q = float(r.choice([1.0, 0.25, 1 / 256]))
    flow = np.round((r.rand(N, ch, H, W) - 0.5) * 16) * q
    for f in range(N):
        if N > 1 and f == 0:
            continue                                                # one NaN-free frame
        for c in range(ch):
            m = flow[f, c]
            flat = m.reshape(-1)
            cnt = int(r.randint(0, max(2, W * H // 4)))
            flat[r.randint(0, W * H, cnt)] = r.choice([NAN, NAN, INF, -INF, 0.0, -0.0, 1e300, -1e300, 5e-324], cnt)
            if r.rand() < 0.5:
                m[r.randint(0, H, int(r.randint(1, 4)))] = NAN
            if r.rand() < 0.4:
                m[:, r.randint(0, W, int(r.randint(1, 4)))] = NAN
            if r.rand() < 0.4:
                y0, x0 = r.randint(0, H), r.randint(0, W)
                m[y0:y0 + int(r.randint(2, 7)), x0:x0 + int(r.randint(2, 7))] = NAN
    return flow


# ------------------------------------------------------------------------------------------------ epipolar geometries
def _rot(ax, ay, az):
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def epi_geometry(r, W, H, oracle=None):
    """(F, Hm, epipole, direction, kind): a random rotation (none: H = I exactly), an epipole inside the image, outside it or far
    away (nearly parallel lines), either direction flag; with an oracle given, now and then the epipole moved onto one pixel's
    Pd0 (F kept), so that that pixel's offset is 0 and its direction 0/0 = NaN."""
    f = float(r.choice([0.58, 1.0, 2.5])) * max(W, H, 8)
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    if r.rand() < 0.25:
        Hm = np.eye(3)
    else:
        Hm = K @ _rot(*((r.rand(3) - 0.5) * float(r.choice([0.002, 0.02, 0.2])))) @ np.linalg.inv(K)
    where = str(r.choice(["inside", "outside", "far", "on_pixel"]))
    if where == "inside":
        e = np.array([r.rand() * W + 0.5, r.rand() * H + 0.5])
    elif where == "outside":
        e = np.array([W * (1.5 + r.rand()) * r.choice([-1, 1]), H * (r.rand() * 3 - 1)])
    else:
        e = np.array([(r.rand() - 0.5) * 1e7, (r.rand() - 0.5) * 1e7])
    E = np.array([e[0], e[1], 1.0])
    ex = np.array([[0, -E[2], E[1]], [E[2], 0, -E[0]], [-E[1], E[0], 0]])
    F = ex @ Hm
    F = F / np.abs(F).max()
    direction = int(r.rand() < 0.5)
    epi = (float(e[0]), float(e[1]))
    if where == "on_pixel":
        if oracle is None:
            where = "inside"
        else:
            Pd0 = oracle.epipolar_maps(F, Hm, epi, direction, W, H)[0]
            y, x = int(r.randint(0, H)), int(r.randint(0, W))
            epi = (float(Pd0[0, y, x]), float(Pd0[1, y, x]))
    return F, Hm, epi, direction, where


EPI_EDGES = (1, 1, 2, 3, 5, 16, 17, 63, 64, 65)


def epi_shape(r, hi=96):
    W, H = pick_size(r, 1, hi, EPI_EDGES), pick_size(r, 1, hi, EPI_EDGES)
    if r.rand() < 0.2:
        W, H = (1, H) if r.rand() < 0.5 else (W, 1)
    return W, H


def epi_random_case(seed, oracle):
    """The draws of tests/test_gpu_edge_sweeps.py::test_epipolar_random_geometries, in its order (shared with the comparison of
    the oracle against the reference's compiled code, tests/ref_cases.py): (r, W, H, D, vMax, paths, ch, B, geos, pairs); r is
    the generator after these draws."""
    r = rng(3000 + seed)
    W, H = epi_shape(r, hi=80)
    D, vMax, paths = int(r.choice([16, 20, 32, 48, 64, 128])), float(r.choice([0.3, 0.5, 0.125])), int(r.choice([4, 8]))
    ch = int(r.choice([1, 3]))
    B = int(r.randint(1, 5))
    geos = [epi_geometry(r, W, H, oracle) for _ in range(B)]
    pairs = [image_pair(r, W, H, ch, seed=seed * 10 + f) for f in range(B)]
    return r, W, H, D, vMax, paths, ch, B, geos, pairs


# ------------------------------------------------------------------------------------------------ oracle compositions
def oracle_flow_pp_frame(oracle, I0, I1, geo, paths, D, vMax):
    """test.m:32-54 composed from the oracle's pieces (the MEX's vz index for D1): (flow, flow2, D1, minC)."""
    H, W = I0.shape[-2:]
    pd0, nd, off, rflow = oracle.epipolar_maps(*geo, W, H)
    if I0.ndim == 3:
        I0, I1 = oracle.rgb2gray(I0), oracle.rgb2gray(I1)
    S = oracle.epi_aggregate(oracle.epi_cost(I0, I1, D, vMax, pd0, nd, off), 6, 64, paths)
    bestD, minC = oracle.epi_wta(S, W, H, D, 1)
    D1 = bestD.astype(np.float64) / 256.0
    flow = np.empty((3, H, W))
    flow[:2] = oracle.vzind2disp(D1, off, vMax, D + 1) * nd + rflow
    flow[2] = 1.0
    f1, _, _ = oracle.postprocess(D1, pd0, nd, off, vMax, D + 1, D)
    flow2 = np.empty((3, H, W))
    flow2[:2] = oracle.vzind2disp(f1, off, vMax, D + 1) * nd + rflow
    flow2[2] = ~np.isnan(f1)
    return flow, flow2, D1, minC


def oracle_pyramidal_ng(oracle, I0, I1, numPyd, half=1, agg=2, sub=0, P1=6, P2=32):
    """The level loop of pyramidal_sgm.m (:24-76) around the oracle's calc_pyd_cost_sgm_ng: impyramid 'reduce' / rgb2gray levels,
    hints 2 * imresize(flow, 2, 'nearest') (:72).  Returns ([flow per level, coarsest first], minC of level 1)."""
    rgb = I0.ndim == 3
    lv = [(I0, I1)]
    for _ in range(1, numPyd):
        a, b = lv[-1]
        red = (lambda im: np.stack([oracle.impyramid_reduce(c) for c in im])) if rgb else oracle.impyramid_reduce
        lv.append((red(a), red(b)))
    gray = [(oracle.rgb2gray(a), oracle.rgb2gray(b)) if rgb else (a, b) for a, b in lv]
    hc, wc = gray[-1][0].shape
    mvPre = np.zeros((2, hc, wc))
    flows = []
    for l in range(numPyd, 0, -1):
        mc, fl = oracle.calc_pyd_cost_sgm_ng(gray[l - 1][0], gray[l - 1][1], mvPre, half, agg, sub, P1, P2)
        flows.append(fl)
        mvPre = np.ascontiguousarray(2.0 * np.repeat(np.repeat(fl, 2, axis=1), 2, axis=2))
    return flows, mc


def image_pair(r, W, H, ch, seed):
    """A uint8 pair (gray or RGB) with a random share of flat and saturated areas."""
    I0, I1 = synth.image_pair(W, H, 12, seed=seed)
    if r.rand() < 0.3:
        I0 = (I0.astype(np.int32) * 5 % 256).astype(np.uint8)
    if r.rand() < 0.2:
        I1 = I1.copy()
        I1[: max(1, H // 3)] = 255
    if ch == 3:
        n0 = synth.uniform_u8(seed + 50, (3, H, W), hi=40).astype(np.int32)
        rgb = lambda I: np.clip(np.stack([I, I // 2 + 60, 255 - I]).astype(np.int32) + n0 - 20, 0, 255).astype(np.uint8)  # noqa: E731
        return rgb(I0), rgb(I1)
    return I0, I1
