"""Test helper: the disturbance rule of include/dmpc_hip.h (dmpc_set_disturbance) restated in numpy / plain Python floats -- every operation an
fp64 operation rounded on its own -- over the counter-based stream of oracle/generators.py.  dmpc_disturbance_sample, the device and this file
must agree bit for bit."""
import numpy as np

from oracle.generators import Stream


def _u(seed, s, i, k):
    """u_0 .. u_5 of scene s, agent i, column k"""
    st = Stream(int(seed), (int(s) << 32) | int(i))
    st.ctr = 6 * int(k)
    return [2.0 * st.draw() - 1.0 for _ in range(6)]


def sample(h, S, n_cmd, k, noise_p=0.0, noise_v=0.0, wind=None, pushes=None, seed=0):
    """(dp, dv), [S,n_cmd,3] each, of column k.  wind None, [3] or [S,3]; pushes None or [n,9]: scene, agent, column, dp, dv."""
    dp, dv = np.zeros((S, n_cmd, 3)), np.zeros((S, n_cmd, 3))
    if k == 0:
        return dp, dv
    h, noise_p, noise_v = float(h), float(noise_p), float(noise_v)
    w = np.zeros((S, 3)) if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64).reshape(-1, 3), (S, 3))
    pushes = [] if pushes is None else [[float(x) for x in row] for row in np.asarray(pushes, dtype=np.float64).reshape(-1, 9)]
    hh = (0.5 * h) * h
    for s in range(S):
        for i in range(n_cmd):
            u = _u(seed, s, i, k) if (noise_p > 0 or noise_v > 0) else None
            for c in range(3):
                wc = float(w[s, c])
                p, v = hh * wc, h * wc
                if noise_p > 0:
                    p = p + noise_p * u[c]
                if noise_v > 0:
                    v = v + noise_v * u[3 + c]
                for q in pushes:   # list order
                    if (int(q[0]), int(q[1]), int(q[2])) == (s, i, k):
                        p, v = p + q[3 + c], v + q[6 + c]
                dp[s, i, c], dv[s, i, c] = p, v
    return dp, dv


def push(scene, agent, column, dp=(0, 0, 0), dv=(0, 0, 0)):
    """one row of pushes"""
    return [scene, agent, column, *dp, *dv]
