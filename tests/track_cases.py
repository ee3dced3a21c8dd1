"""Seeded measurement sequences for the tracker tests (CPU and GPU share them).

A sequence is a list of calls; each call is one evaluation time for `rows`
streams out of S: (stream_of_row [rows] int32, t_us [rows] int64,
count [rows] int32, xy [rows][Kp][2] float32).  Per stream two constant-velocity
sources cross near the origin; measurements carry noise, drop out, come with
clutter (sometimes more of it than there are free slots), are sometimes NaN;
some rows are skipped (count <= 0), counts past Kp are clamped, one gap is
longer than max_coast_us and the rows name the streams in a fresh permutation
every call.  The last stream follows a script that makes two exact ties (two
tracks for one measurement, two measurements for one track) where the shape
has room for it (T >= 2 and Kp >= 2).  Magnitudes stay within [1e-3, 1e7].
"""
import numpy as np

HOP_US = 10240  # 512 samples at 50 kHz
SHAPES = [(8, 8), (1, 1), (1, 8), (8, 1), (3, 5)]  # (T, Kp)
SEEDS = (11, 12)

# what the sequences run with: short lives so every event kind turns up
PARAMS = dict(confirm_hits=3, max_misses=3, max_coast_us=400_000, gate_d2=9.0, meas_var=0.01, accel_psd=1.0,
              init_vel_var=4.0)


def make_sequence(seed, T, Kp, S=6, rows=6, evals=60, gap_at=None):
    rng = np.random.default_rng([seed, T, Kp, S, rows])
    gap_at = evals // 2 if gap_at is None else gap_at
    v = rng.uniform(0.5, 1.5, (S, 2)) * rng.choice([-1.0, 1.0], (S, 2))
    y0 = rng.uniform(-0.5, 0.5, (S, 2))
    script = S - 1 if (T >= 2 and Kp >= 2 and S > 1) else -1
    calls, t = [], 0
    for e in range(evals):
        t += HOP_US * (1 + int(rng.integers(0, 2)))
        if e == gap_at:
            t += 1_000_000  # longer than max_coast_us: every track coasts out
        streams = rng.permutation(S)[:rows].astype(np.int32)
        xy = np.full((rows, Kp, 2), 1e6, np.float32)  # past the count: never read
        count = np.zeros(rows, np.int32)
        for i, s in enumerate(streams):
            if s == script and e < 6:
                z = {0: [(-0.125, 0.0), (0.125, 0.0)],  # two tracks born side by side
                     1: [(0.0, 0.0)],                   # ... tie for one measurement
                     2: [(float("nan"), 0.0)],          # evaluated rows without a valid measurement:
                     3: [(float("nan"), 0.0)],          # both tracks miss out
                     4: [(float("nan"), 0.0)],
                     5: [(2.0, 2.0)]}[e]                # a lone track at (2, 2) ...
            elif s == script and e == 6:
                z = [(2.125, 2.0), (1.875, 2.0)]        # ... and two measurements tie for it
            else:
                tt = (t - 300_000) * 1e-6
                z = []
                for a in range(2):
                    if rng.random() > 0.2:  # else: a dropout
                        z.append((v[s, a] * tt * (1 if a == 0 else 0.7) + rng.normal(0, 0.03),
                                  y0[s, a] + 0.3 * v[s, 1 - a] * tt + rng.normal(0, 0.03)))
                nclutter = int(rng.choice([0, 0, 0, 1, 2, Kp]))
                z += [tuple(rng.uniform(-2.0, 2.0, 2)) for _ in range(nclutter)]
                if rng.random() < 0.08 and z:
                    z[int(rng.integers(len(z)))] = (float("nan"), 0.5)
                if rng.random() < 0.05 and z:
                    z[int(rng.integers(len(z)))] = (0.25, float("inf"))
                z = [z[k] for k in rng.permutation(len(z))][:Kp]
                if rng.random() < 0.1:
                    z = []  # a skipped row
            n = len(z)
            if n:
                xy[i, :n] = np.asarray(z, np.float32)
            count[i] = n
            if n == 0 and rng.random() < 0.5:
                count[i] = -3
            if n == Kp and rng.random() < 0.5:
                count[i] = Kp + 2  # clamped to Kp
        calls.append((streams, np.full(rows, t, np.int64), count, xy))
    return calls


def params(T):
    return dict(PARAMS, max_tracks=T)
