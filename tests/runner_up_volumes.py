"""Cost volumes for the runner-up tests: seeded-random u8 <= 24 with crafted rows, and the edge counts a test must meet.

With penalties (P1, P2) = (3, 10) a crafted pixel -- cost 0 at its target d, 1 at one neighbour of it, 12..24 elsewhere --
keeps a path cost <= 10 at the target, <= 11 at that neighbour and >= 12 everywhere else, on every path: the minimum of S lies at
the target or the neighbour, and the other of the two is the global second minimum, next to the winner.
"""
import numpy as np

from tests import runner_up_restatement as RU

W, H = 37, 19                       # 703 pixels: a multiple of no pixels-per-block count of the WTA kernels
P1, P2 = 3, 10
PACKED = {16: (1, 16), 32: (2, 16), 64: (4, 16), 128: (8, 16), 256: (16, 16)}
SPLIT = {48: (4, 12), 96: (8, 12), 192: (16, 12), 80: (4, 20), 160: (8, 20), 112: (4, 28), 224: (8, 28)}
GENERIC = (1, 2, 3, 5, 20, 144, 300, 1024)
ALL_D = tuple(PACKED) + tuple(SPLIT) + GENERIC


def split_of(D):
    """(lanes per pixel, costs per lane) of the packed WTA at this range; (0, 0): the generic kernel"""
    return PACKED.get(D) or SPLIT.get(D) or (0, 0)


def boundaries(D):
    """the d on a lane boundary: j * DPL and j * DPL - 1 of the range's split; the generic kernel's lanes stride over d, so its
    wave boundary 64 k stands in"""
    lpp, dpl = split_of(D)
    step = dpl if lpp else 64
    return sorted({d for j in range(1, (D + step - 1) // step) for d in (j * step - 1, j * step) if 0 <= d < D})


def targets(D):
    if D <= 5:
        return list(range(D))
    return sorted(set(boundaries(D)) | {D // 2})


def volume(D, seed, constant=False):
    """u8 [H][W][D] <= 24.  constant: every pixel's cost is one value for all d (S is then constant in d: best = 0).  Else row 0
    constant in d, row 1 the single minimum at d = 0, row 2 at D - 1, rows 3.. at the targets in runs of four pixels, their second
    smallest cost beside them (left and right in turn), the last four rows plain noise."""
    rng = np.random.default_rng(seed)
    if constant:
        return np.ascontiguousarray(np.repeat(rng.integers(0, 25, (H, W, 1)), D, axis=2).astype(np.uint8))
    C = rng.integers(0, 25, (H, W, D)).astype(np.uint8)
    C[0] = rng.integers(0, 25, (W, 1))
    T = targets(D)
    for y in range(1, H - 4):
        for x in range(W):
            t = 0 if y == 1 else D - 1 if y == 2 else T[(x // 4 + 3 * y) % len(T)]
            C[y, x] = rng.integers(12, 25, D)
            C[y, x, t] = 0
            side = t + (1 if (x + y) % 2 else -1)
            if not 0 <= side < D:
                side = t - (side - t)
            if 0 <= side < D:
                C[y, x, side] = 1
    return np.ascontiguousarray(C)


def volumes(D, batch, seed):
    """the frames of a batch: crafted ones, the last of three constant in d throughout"""
    return [volume(D, seed + f, constant=(batch == 3 and f == 2)) for f in range(batch)]


def edge_counts(D, best, minC, minC2, S):
    """from the expected arrays alone: how many pixels meet each edge"""
    S = np.asarray(S).reshape(-1, D).astype(np.int64)
    best, minC2 = np.asarray(best).ravel(), np.asarray(minC2).ravel().astype(np.int64)
    big = np.int64(1) << 40
    left = np.where(best > 0, S[np.arange(len(best)), np.maximum(best - 1, 0)], big)
    right = np.where(best < D - 1, S[np.arange(len(best)), np.minimum(best + 1, D - 1)], big)
    return {"best_first": int((best == 0).sum()), "best_last": int((best == D - 1).sum()),
            "boundary": int(np.isin(best, boundaries(D)).sum()),
            "adjacent_second": int((np.minimum(left, right) < minC2).sum()),     # (NO_RUNNER_UP counts: the only other costs are adjacent)
            "none": int((minC2 == RU.NO_RUNNER_UP).sum()),
            "tie": int((minC2 == np.asarray(minC).ravel()).sum())}


def required(D, batch):
    """the counts that can be non-zero at this range and batch, and so must be"""
    need = ["best_first", "best_last"]
    if split_of(D)[0] > 1 or (not split_of(D)[0] and D > 64):
        need.append("boundary")
    if D >= 2:
        need.append("adjacent_second")
    if D <= 3:
        need.append("none")
    if D >= 3 and batch == 3:
        need.append("tie")                                       # the frame that is constant in d: minC2 == minC
    return need
