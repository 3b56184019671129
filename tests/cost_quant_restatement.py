"""The quantising rule of the float cost-volume entries (include/fsgm.h, "Float cost volumes"), restated in numpy: the yardstick
of tests/test_sgm_float_cpu.py and tests/test_gpu_sgm_float.py.  Every step is one numpy operation on float32 arrays, so each
rounds once, to nearest even, as the rule demands; nothing here can contract the multiply and the add."""
import numpy as np


def quantise(x, scale, offset, bound):
    """x: the volume widened to float32 (exact for float16 and bfloat16: widen before calling); scale, offset: rounded to float32
    here, as the C struct holds them; bound: the call's cost_bound, 1..255.  Returns (q uint8, flagged bool), both of x's shape."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and 1 <= int(bound) <= 255
    scale, offset, B = np.float32(scale), np.float32(offset), np.float32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.multiply(x, scale, dtype=np.float32)          # 2. one fp32 multiply
        u = np.add(t, offset, dtype=np.float32)              # 3. one fp32 add
        r = np.rint(u)                                       # 4. ties to even
        low, high = r < 0, (r > B) | np.isnan(u)             # 5. (-0.0 < 0 is False)
        q = np.where(low, np.float32(0), np.where(high, B, r)).astype(np.uint8)
    return q, low | high
