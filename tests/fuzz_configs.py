"""The configuration draws of the seeded random sweeps (tests/test_gpu_fuzz.py), shared with the CPU comparison of the oracle
against the reference's compiled MEX code (tests/test_oracle_ref_parity.py): one seed gives both the same configuration.

Each function consumes its RandomState in a fixed order; the order is part of the test suite's definition."""
import numpy as np


def rng(seed):
    return np.random.RandomState(seed)          # only picks test configurations; data comes from synth


def epi_config(seed):
    """test_epi_random_configs: dict(D, W, H, paths, P1, P2, cmax, sub, vz, B)."""
    r = rng(seed)
    D = int(r.choice([16, 32, 64, 128, 256, 8, 20, 48, 100]))
    W, H = int(r.randint(1, 90)), int(r.randint(1, 70))
    paths = int(r.choice([4, 8]))
    if r.rand() < 0.6:
        P1, P2, cmax = int(r.randint(0, 20)), int(r.randint(0, 86)), 24        # no-wrap side
    else:
        P1, P2, cmax = int(r.randint(0, 256)), int(r.randint(0, 256)), int(r.choice([24, 255]))
    sub, vz = int(r.rand() < 0.7), int(r.rand() < 0.5)
    B = int(r.choice([1, 2, 5]))
    return dict(D=D, W=W, H=H, paths=paths, P1=P1, P2=P2, cmax=cmax, sub=sub, vz=vz, B=B)


def epi_tall_config(seed):
    """test_epi_random_tall_configs: dict(D, W, H, paths, P1, P2, sub, vz, B)."""
    r = rng(500 + seed)
    D = int(r.choice([16, 32, 64, 128, 128, 256]))
    W, H = int(r.randint(1, 40)), int(r.randint(60, 330))
    paths = int(r.choice([4, 8]))
    P1 = int(r.randint(0, 30))
    P2 = int(r.randint(P1, 100))                            # P1 <= P2; some beyond the fused kernels' byte budgets
    sub, vz = int(r.rand() < 0.7), int(r.rand() < 0.5)
    B = int(r.choice([1, 2, 3]))
    return dict(D=D, W=W, H=H, paths=paths, P1=P1, P2=P2, sub=sub, vz=vz, B=B)


def pyd_config(seed):
    """test_pyd_random_configs: dict(W, H, rX, rY, rAgg, mvW, mvH, kind, P1, P2, diag, passes, adaptive, sub, amp)."""
    r = rng(100 + seed)
    W, H = int(r.randint(1, 60)), int(r.randint(1, 45))
    rX, rY, rAgg = int(r.randint(0, 6)), int(r.randint(0, 6)), int(r.randint(0, 4))
    mvW, mvH = W + int(r.randint(0, 4)), H + int(r.randint(0, 4))
    kind = str(r.choice(["zero", "even", "general"]))
    P1, P2 = (6, 32) if r.rand() < 0.6 else (int(r.randint(0, 256)), int(r.randint(0, 256)))
    diag, passes, adaptive, sub = int(r.rand() < 0.7), int(r.choice([1, 2, 2, 3])), int(r.rand() < 0.5), int(r.rand() < 0.5)
    amp = float(r.choice([1.5, 4.0, 9.0]))
    return dict(W=W, H=H, rX=rX, rY=rY, rAgg=rAgg, mvW=mvW, mvH=mvH, kind=kind, P1=P1, P2=P2, diag=diag, passes=passes,
                adaptive=adaptive, sub=sub, amp=amp)


def ng_config(seed):
    """test_ng_random_configs: dict(W, H, mvW, mvH, P1, P2, half, agg, sub, kind, amp)."""
    r = rng(200 + seed)
    W, H = int(r.randint(1, 40)), int(r.randint(1, 30))
    mvW, mvH = int(r.randint(1, W + 3)), int(r.randint(1, H + 3))
    P1, P2 = (6, 32) if r.rand() < 0.5 else (int(r.randint(0, 256)), int(r.randint(0, 256)))
    half, agg, sub = int(r.choice([0, 1, 1, 2])), int(r.randint(0, 6)), int(r.rand() < 0.5)
    kind, amp = str(r.choice(["zero", "even", "int", "general"])), float(r.choice([0.7, 2.0, 6.0]))   # few to many repeated candidates
    return dict(W=W, H=H, mvW=mvW, mvH=mvH, P1=P1, P2=P2, half=half, agg=agg, sub=sub, kind=kind, amp=amp)
