"""development: are the arrays of two .npz dumps identical bit for bit?   usage: python tools/npz_equal.py a.npz b.npz [skip-substring ...]"""
import sys
import numpy as np
a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
skip = sys.argv[3:]
bad = 0
for k in a.files:
    if any(s in k for s in skip): continue
    x, y = a[k], b[k]
    if k.startswith("info"): x, y = x[..., :4], y[..., :4]   # (branch record; iteration statistics may differ between builds)
    if x.dtype != y.dtype or x.shape != y.shape or np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():   # (bytes: NaN equals NaN)
        bad += 1
        d = np.nanmax(np.abs(x.astype(float) - y.astype(float))) if x.shape == y.shape and x.size else np.nan
        print(f"{k}: differs (max abs {d:.3e})")
print("identical" if not bad else f"{bad} arrays differ", f"({len(a.files)} arrays)")
