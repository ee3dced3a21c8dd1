"""The tracker's rule (include/tdoa.h, "Tracking") restated in numpy: the
reference tdoa_track_host, tdoa_track_batch and tdoa_stream_track are held to,
bit for bit.

Every float is an np.float32 scalar and every expression one operation, so each
result is rounded to fp32 on its own; times are np.int64 and become float by
np.float32(np.int64).  Steps, per evaluated row (stream s, time t, n = count
clamped to [0, Kp], measurements z_k, k < n; T = max_tracks, r = meas_var,
q = accel_psd):

  0. n <= 0: the row is not evaluated (state untouched, outputs = the unchanged
     table, assigned all 0).  A measurement with a non-finite coordinate is
     invalid: neither associated nor born.
  1. coast-out: live slot j < T with t - upd_us > max_coast_us is zeroed.
  2. predict every live track: dt = (float)max(t - t_us, 0) / 1e6f;
     x += vx*dt; y += vy*dt; a = dt*p11; c = (p01 + p01) + a; d = dt*c;
     dt2 = dt*dt; dt3 = dt2*dt; p00 = (p00 + d) + (q*dt3)/3; p01 = (p01 + a) +
     (q*dt2)*0.5; p11 = p11 + q*dt; t_us = t.
  3. cost for live j, valid k: dx = zx - x; dy = zy - y; s = p00 + r;
     c_jk = (dx*dx + dy*dy) / s; eligible iff c_jk <= gate_d2.
  4. greedy: the eligible pair of minimum c among unassigned tracks and
     measurements, ties to the lowest j then the lowest k, until none remains.
  5. assigned track, from the old values: k0 = p00/s; k1 = p01/s; x += k0*dx;
     y += k0*dy; vx += k1*dx; vy += k1*dy; p11 -= k1*p01; p01 -= k0*p01;
     p00 -= k0*p00; hits += 1; misses = 0; upd_us = t; peak = k; tentative and
     hits >= confirm_hits -> confirmed.
  6. unassigned live track: misses += 1; peak = -1; misses >= max_misses frees it.
  7. births: each unassigned valid measurement in ascending k takes the lowest
     free slot < T, or is dropped; id = ++next_id[s], status = 2 if
     confirm_hits <= 1 else 1, hits 1, misses 0, (x, y) = z, v = 0, p00 = r,
     p01 = 0, p11 = init_vel_var, t_us = upd_us = t, peak = k.
"""
import numpy as np

MAX_TRACKS = 8
F = np.float32

TRACK_DTYPE = np.dtype([("id", "<i4"), ("status", "<i4"), ("hits", "<i4"), ("misses", "<i4"),
                        ("x", "<f4"), ("y", "<f4"), ("vx", "<f4"), ("vy", "<f4"),
                        ("p00", "<f4"), ("p01", "<f4"), ("p11", "<f4"), ("peak", "<i4"),
                        ("t_us", "<i8"), ("upd_us", "<i8")])

DEFAULTS = dict(max_tracks=8, confirm_hits=3, max_misses=5, max_coast_us=2_000_000, gate_d2=9.0,
                meas_var=0.01, accel_psd=1.0, init_vel_var=4.0)

EVENTS = ("births", "confirmations", "miss_outs", "coast_outs", "dropped", "gate_rejections", "tie_breaks",
          "rows_skipped")


def new_tally():
    return {e: 0 for e in EVENTS}


def new_state(S):
    return np.zeros((S, MAX_TRACKS), TRACK_DTYPE), np.zeros(S, np.int32)


def _predict(tr, t, q):
    el = np.int64(t) - np.int64(tr["t_us"])
    dt = F(np.int64(max(int(el), 0))) / F(1e6)
    mx = tr["vx"] * dt
    my = tr["vy"] * dt
    tr["x"] = tr["x"] + mx
    tr["y"] = tr["y"] + my
    a = dt * tr["p11"]
    p2 = tr["p01"] + tr["p01"]
    c = p2 + a
    d = dt * c
    dt2 = dt * dt
    dt3 = dt2 * dt
    q3 = q * dt3
    q2 = q * dt2
    q1 = q * dt
    e0 = tr["p00"] + d
    e1 = tr["p01"] + a
    t3 = q3 / F(3.0)
    h2 = q2 * F(0.5)
    tr["p00"] = e0 + t3
    tr["p01"] = e1 + h2
    tr["p11"] = tr["p11"] + q1
    tr["t_us"] = t


def _row(tr, next_id, t, n, z, p, tally):
    """One evaluated row on the table tr [8] (in place); returns (next_id, assigned [n])."""
    T = p["max_tracks"]
    r, q, gate = F(p["meas_var"]), F(p["accel_psd"]), F(p["gate_d2"])
    asg = np.zeros(n, np.int32)
    valid = [bool(np.isfinite(z[k, 0]) and np.isfinite(z[k, 1])) for k in range(n)]
    for j in range(T):
        if tr[j]["id"] != 0 and int(t) - int(tr[j]["upd_us"]) > p["max_coast_us"]:
            tr[j] = np.zeros((), TRACK_DTYPE)
            tally["coast_outs"] += 1
    live = [bool(tr[j]["id"] != 0) for j in range(T)]
    cost, inn, sv = {}, {}, {}
    for j in range(T):
        if not live[j]:
            continue
        _predict(tr[j], t, q)
        for k in range(n):
            if not valid[k]:
                continue
            dx = F(z[k, 0]) - tr[j]["x"]
            dy = F(z[k, 1]) - tr[j]["y"]
            s = tr[j]["p00"] + r
            xx = dx * dx
            yy = dy * dy
            d2 = xx + yy
            c = d2 / s
            sv[j] = s
            if c <= gate:
                cost[(j, k)] = c
                inn[(j, k)] = (dx, dy)
            else:
                tally["gate_rejections"] += 1
    got, used = {}, set()
    while True:
        cand = [(j, k) for (j, k) in sorted(cost) if j not in got and k not in used]
        if not cand:
            break
        best = cand[0]
        for jk in cand[1:]:
            if cost[jk] < cost[best]:
                best = jk
        if sum(1 for jk in cand if cost[jk] == cost[best]) > 1:
            tally["tie_breaks"] += 1
        got[best[0]] = best[1]
        used.add(best[1])
    for j in range(T):
        if not live[j]:
            continue
        t_ = tr[j]
        if j in got:
            k = got[j]
            dx, dy = inn[(j, k)]
            s = sv[j]
            k0 = t_["p00"] / s
            k1 = t_["p01"] / s
            ax = k0 * dx
            ay = k0 * dy
            bx = k1 * dx
            by = k1 * dy
            t_["x"] = t_["x"] + ax
            t_["y"] = t_["y"] + ay
            t_["vx"] = t_["vx"] + bx
            t_["vy"] = t_["vy"] + by
            m11 = k1 * t_["p01"]
            m01 = k0 * t_["p01"]
            m00 = k0 * t_["p00"]
            t_["p11"] = t_["p11"] - m11
            t_["p01"] = t_["p01"] - m01
            t_["p00"] = t_["p00"] - m00
            t_["hits"] += 1
            t_["misses"] = 0
            t_["upd_us"] = t
            t_["peak"] = k
            if t_["status"] == 1 and t_["hits"] >= p["confirm_hits"]:
                t_["status"] = 2
                tally["confirmations"] += 1
            asg[k] = t_["id"]
        else:
            t_["misses"] += 1
            t_["peak"] = -1
            if t_["misses"] >= p["max_misses"]:
                tr[j] = np.zeros((), TRACK_DTYPE)
                tally["miss_outs"] += 1
    for k in range(n):
        if not valid[k] or k in used:
            continue
        free = [j for j in range(T) if tr[j]["id"] == 0]
        if not free:
            tally["dropped"] += 1
            continue
        next_id = np.int32(next_id + 1)
        b = tr[free[0]]
        b["id"] = next_id
        b["status"] = 2 if p["confirm_hits"] <= 1 else 1
        b["hits"] = 1
        b["misses"] = 0
        b["x"], b["y"] = F(z[k, 0]), F(z[k, 1])
        b["vx"] = b["vy"] = F(0)
        b["p00"], b["p01"], b["p11"] = r, F(0), F(p["init_vel_var"])
        b["peak"] = k
        b["t_us"] = b["upd_us"] = t
        asg[k] = next_id
        tally["births"] += 1
        if b["status"] == 2:
            tally["confirmations"] += 1
    return next_id, asg


def track_rows(tracks, next_id, t_us, count, xy, stream_of_row=None, tally=None, **params):
    """The rows of one call, in order.  tracks [S][8] TRACK_DTYPE and next_id [S]
    are not modified; returns (tracks, next_id, out, tally) with out = tracks
    [rows][T], assigned [rows][Kp], num_confirmed [rows]."""
    p = {**DEFAULTS, **params}
    tracks, next_id = tracks.copy(), next_id.copy()
    tally = new_tally() if tally is None else tally
    xy = np.asarray(xy, np.float32)
    rows, Kp = xy.shape[0], xy.shape[1]
    T = p["max_tracks"]
    out = {"tracks": np.zeros((rows, T), TRACK_DTYPE), "assigned": np.zeros((rows, Kp), np.int32),
           "num_confirmed": np.zeros(rows, np.int32)}
    with np.errstate(all="ignore"):
        for i in range(rows):
            s = int(stream_of_row[i]) if stream_of_row is not None else i
            n = min(max(int(count[i]), 0), Kp)
            if n > 0:
                next_id[s], asg = _row(tracks[s], next_id[s], np.int64(t_us[i]), n, xy[i], p, tally)
                out["assigned"][i, :n] = asg
            else:
                tally["rows_skipped"] += 1
            out["tracks"][i] = tracks[s, :T]
            out["num_confirmed"][i] = int((tracks[s, :T]["status"] == 2).sum())
    return tracks, next_id, out, tally
