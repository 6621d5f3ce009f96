"""A numpy restatement, in binary32, of the blur, the gradient and one descriptor of "Describing given SIFT frames"
(include/msfm.h).  It is written array-wise where tests/sift_ref.cpp walks pixel by pixel, and guards that program against a
misreading the two would otherwise share.  Every constant is wrapped in F32 so that no operation widens; the numbers that need
exp, pow, log2, fmod, sin or cos come from `host_numbers` / `frame_records` below, computed with the C library through `math`
exactly as metricsfm_amd/csrc/sift_args.h does."""
import math

import numpy as np

F32 = np.float32
EPS = F32(1.19209290e-07)
PI2 = F32(6.28318548)
C_ATAN = [F32(c) for c in (0.99997726, -0.33262347, 0.19354346, -0.11643287, 0.05265332, -0.01172120)]
FRAME_DT = np.dtype([("x", F32), ("y", F32), ("sigma", F32), ("thr", F32), ("st", F32), ("ct", F32), ("o", np.int32), ("is", np.int32)])


# ---- host numbers (binary64, the C library's functions, rounded once) ----
def level_blur(S, s):
    k = math.pow(2.0, 1.0 / S)
    sigma0 = 1.6 * k
    if s < 0:
        sa = sigma0 * math.pow(k, -1.0)
        return math.sqrt(sa * sa - 0.25)
    return sigma0 * math.sqrt(1 - 1 / (k * k)) * math.pow(k, float(s))


def taps_of(sd):
    W = max(int(math.ceil(4 * sd)), 1)
    g = [math.exp(-0.5 * (float(i - W) * float(i - W)) / (sd * sd)) for i in range(2 * W + 1)]
    total = 0.0
    for v in g:
        total += v
    return np.array([v / total for v in g], np.float64).astype(F32)


def host_numbers(S):
    """-> (the S + 3 tap arrays of the levels -1 .. S + 1, the window table T[257])"""
    return [taps_of(level_blur(S, s)) for s in range(-1, S + 2)], np.array([math.exp(-i * 25.0 / 256.0) for i in range(257)], np.float64).astype(F32)


def frame_records(frames, O, S):
    """frames [n][4] float32 (x, y, sigma, theta) -> the records the descriptor takes (FRAME_DT)"""
    frames = np.asarray(frames, F32).reshape(-1, 4)
    rec = np.zeros(len(frames), FRAME_DT)
    sigma0 = 1.6 * math.pow(2.0, 1.0 / S)
    two_pi = 6.283185307179586
    for f, (x, y, sg, th) in enumerate(frames):
        phi = math.log2((float(sg) + 1.1920928955078125e-07) / sigma0)
        o = min(max(math.floor(phi - (-1 + 0.5) / S), 0), O - 1)
        i_s = min(max(math.floor(S * (phi - o) + 0.5), 0), S - 1)
        thr = math.fmod(float(th), two_pi)
        if thr < 0:
            thr += two_pi
        rec[f] = (x, y, sg, F32(thr), F32(math.sin(float(th))), F32(math.cos(float(th))), o, i_s)
    return rec


# ---- binary32 arithmetic ----
def stretch(img):
    v = np.asarray(img, np.uint8)
    lo, hi = int(v.min()), int(v.max())
    return (v.astype(F32) - F32(lo)) / F32(hi - lo) * F32(255.0)


def blur(src, g):
    W = len(g) // 2
    h, w = src.shape
    ix = np.arange(w)
    rows = np.zeros_like(src)
    for i in range(2 * W + 1):
        rows = rows + g[i] * src[:, np.clip(ix + i - W, 0, w - 1)]
    iy = np.arange(h)
    out = np.zeros_like(src)
    for i in range(2 * W + 1):
        out = out + g[i] * rows[np.clip(iy + i - W, 0, h - 1), :]
    return out


def angle_of(gx, gy):
    ax, ay = np.abs(gx), np.abs(gy)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = mn / mx
    q = t * t
    r = C_ATAN[5]
    for c in C_ATAN[4::-1]:
        r = c + q * r
    r = t * r
    r = np.where(ay > ax, F32(1.57079637) - r, r)
    r = np.where(gx < 0, F32(3.14159274) - r, r)
    r = np.where(gy < 0, PI2 - r, r)
    r = np.where(r >= PI2, r - PI2, r)
    return np.where(mx == 0, F32(0), r).astype(F32)


def gradient(I):
    gx, gy = np.empty_like(I), np.empty_like(I)
    gx[:, 1:-1] = F32(0.5) * (I[:, 2:] - I[:, :-2])
    gx[:, 0], gx[:, -1] = I[:, 1] - I[:, 0], I[:, -1] - I[:, -2]
    gy[1:-1, :] = F32(0.5) * (I[2:, :] - I[:-2, :])
    gy[0, :], gy[-1, :] = I[1, :] - I[0, :], I[-1, :] - I[-2, :]
    return np.sqrt(gx * gx + gy * gy), angle_of(gx, gy)


def scalespace(img, O, S, taps):
    """-> gss[o][s + 1], mod[o][s], ang[o][s]"""
    gss, mod, ang = [], [], []
    for o in range(O):
        lv = [blur(stretch(img), taps[0]) if o == 0 else np.ascontiguousarray(gss[o - 1][S][0:2 * (gss[o - 1][S].shape[0] >> 1):2,
                                                                                        0:2 * (gss[o - 1][S].shape[1] >> 1):2])]
        for s in range(S + 2):
            lv.append(blur(lv[s], taps[s + 1]))
        gss.append(lv)
        gr = [gradient(lv[s + 1]) for s in range(S)]
        mod.append([g[0] for g in gr])
        ang.append([g[1] for g in gr])
    return gss, mod, ang


PERM = np.array([((8 - (b % 8)) % 8) + 8 * ((b // 8) % 4) + 32 * (3 - b // 32) for b in range(128)])   # column of bin b


def _norm(hist):
    s = F32(0)
    for b in range(128):
        s = s + hist[b] * hist[b]
    return np.sqrt(s) + EPS


def describe(F, mod, ang, T, quantize, norms=None):
    """The row of one record F (FRAME_DT) on its level's gradient planes; `norms` (a list) receives the two norms."""
    h, w = mod.shape
    out = np.zeros(128, F32)
    sc = F32(1 << int(F["o"]))
    xp, yp, sp = F["x"] / sc, F["y"] / sc, F["sigma"] / sc
    xf, yf = xp + F32(0.5), yp + F32(0.5)
    if not (xf > -1 and xf < w and yf > -1 and yf < h - 1):
        return out
    xi, yi = int(xf), int(yf)
    SBP = F32(3.0) * sp + EPS
    Wf = np.floor(F32(1.41421356) * SBP * F32(2.5) + F32(0.5))
    W = int(Wf) if Wf < 32768 else 32768
    ys = np.arange(yi + max(-W, 1 - yi), yi + min(W, h - yi - 2) + 1)
    xs = np.arange(xi + max(-W, 1 - xi), xi + min(W, w - xi - 2) + 1)
    hist = np.zeros(128, F32)
    if len(ys) and len(xs):
        px, py = (a.reshape(-1) for a in np.meshgrid(xs, ys))   # raster order: x fastest
        st, ct = F["st"], F["ct"]
        dx, dy = px.astype(F32) - xp, py.astype(F32) - yp
        with np.errstate(over="ignore"):
            nx = (ct * dx + st * dy) / SBP
            ny = ((-st) * dx + ct * dy) / SBP
            u = ((nx * nx + ny * ny) * F32(0.125)) * F32(10.24)
        th = ang[py, px] - F["thr"]
        th = np.where(th < 0, th + PI2, th)
        th = np.where(th >= PI2, th - PI2, th)
        nt = (F32(8.0) * th) / PI2
        bx, by, bt = np.floor(nx - F32(0.5)), np.floor(ny - F32(0.5)), np.floor(nt)
        keep = (u < 256) & (bx >= -3) & (bx <= 1) & (by >= -3) & (by <= 1)
        for k in np.flatnonzero(keep):
            i = int(u[k])
            fr = u[k] - F32(i)
            win = T[i] + fr * (T[i + 1] - T[i])
            base = win * mod[py[k], px[k]]
            rx, ry, rt = nx[k] - (bx[k] + F32(0.5)), ny[k] - (by[k] + F32(0.5)), nt[k] - bt[k]
            wx, wy, wt = (abs(F32(1.0) - rx), abs(rx)), (abs(F32(1.0) - ry), abs(ry)), (abs(F32(1.0) - rt), abs(rt))
            for dby in (0, 1):
                for dbx in (0, 1):
                    cx, cy = int(bx[k]) + dbx, int(by[k]) + dby
                    if cx < -2 or cx > 1 or cy < -2 or cy > 1:
                        continue
                    for dbt in (0, 1):
                        b = (int(bt[k]) + dbt) % 8 + 8 * (cx + 2) + 32 * (cy + 2)
                        hist[b] = hist[b] + ((base * wx[dbx]) * wy[dby]) * wt[dbt]
    n1 = _norm(hist)
    hist = np.minimum(hist / n1, F32(0.2))
    n2 = _norm(hist)
    if norms is not None:
        norms += [n1, n2]
    v = F32(512.0) * (hist / n2)
    if quantize:
        v = np.minimum(v.astype(np.int32).astype(F32), F32(255.0))
    out[PERM] = v
    return out
