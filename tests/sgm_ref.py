"""A second restatement of the dense-stereo definitions of include/msfm.h ("Dense stereo"), in numpy, written from the formulas
and not from tests/sgm_ref.cpp: whole rows, columns and disparity vectors at a time, sorting where the C++ keeps two minima."""
import numpy as np

DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def popcount32(a):
    a = np.ascontiguousarray(a, np.uint32)
    return _POP8[a.view(np.uint8).reshape(a.shape + (4,))].sum(-1).astype(np.int64)


def census(img):
    I = np.asarray(img, np.uint8).astype(np.int64)
    h, w = I.shape
    out = np.zeros((h, w), np.uint32)
    if h < 7 or w < 9:
        return out
    offsets = [(dx, dy) for dy in (-3, -2, -1) for dx in range(-4, 5)] + [(dx, 0) for dx in range(-4, 0)]
    ys, xs = slice(3, h - 3), slice(4, w - 4)
    f = np.zeros((h - 6, w - 8), np.uint32)
    for dx, dy in offsets:
        a = I[3 + dy:h - 3 + dy, 4 + dx:w - 4 + dx]
        b = I[3 - dy:h - 3 - dy, 4 - dx:w - 4 - dx]
        f = (f << np.uint32(1)) | (a > b).astype(np.uint32)
    out[ys, xs] = f
    return out


def matching_cost(cl, cr, D):
    """C [h][w][D]"""
    h, w = cl.shape
    C = np.zeros((h, w, D), np.int64)
    for d in range(D):
        shifted = np.zeros_like(cr)
        shifted[:, d:] = cr[:, :w - d]
        C[:, :, d] = popcount32(cl ^ shifted)
    return C


def _step(prev, C, P1, P2):
    """prev, C [..., D] -> L of the next pixel along the path"""
    m = prev.min(-1, keepdims=True)
    big = np.int64(1 << 40)
    down = np.concatenate([np.full(prev.shape[:-1] + (1,), big), prev[..., :-1]], -1)
    up = np.concatenate([prev[..., 1:], np.full(prev.shape[:-1] + (1,), big)], -1)
    return C + np.minimum(np.minimum(prev - m, P2), np.minimum(down, up) - m + P1)


def path_cost(C, r, P1, P2):
    """L_r [h][w][D] (int64) of direction index r"""
    h, w, D = C.shape
    rx, ry = DIRS[r]
    L = np.zeros_like(C)
    if ry == 0:
        order = range(w) if rx > 0 else range(w - 1, -1, -1)
        for x in order:
            q = x - rx
            L[:, x] = C[:, x] if not 0 <= q < w else _step(L[:, q], C[:, x], P1, P2)
        return L
    order = range(h) if ry > 0 else range(h - 1, -1, -1)
    xs = np.arange(w)
    for y in order:
        qy = y - ry
        if not 0 <= qy < h:
            L[y] = C[y]
            continue
        qx = xs - rx
        ok = (qx >= 0) & (qx < w)
        rec = _step(L[qy][np.clip(qx, 0, w - 1)], C[y], P1, P2)
        L[y] = np.where(ok[:, None], rec, C[y])
    return L


def _decide(keys, uniqueness):
    """keys [..., n] uint64 (0xffffffff: no candidate) -> disparity by the uniqueness rule, from the two smallest"""
    srt = np.sort(keys, -1)
    k0, k1 = srt[..., 0], srt[..., 1]
    c0, d0 = (k0 >> 16).astype(np.int64), (k0 & 0xffff).astype(np.int64)
    c1, d1 = (k1 >> 16).astype(np.int64), (k1 & 0xffff).astype(np.int64)
    product = c1.astype(np.float32) * np.float32(uniqueness)
    keep = (product >= c0.astype(np.float32)) | (np.abs(d1 - d0) <= 1)
    return np.where(keep, d0, 0).astype(np.uint16)


def winners(S, uniqueness):
    """S [h][w][D] -> (raw left, raw right) uint16"""
    h, w, D = S.shape
    d = np.arange(D, dtype=np.uint64)
    left = _decide((S.astype(np.uint64) << np.uint64(16)) | d, uniqueness)
    keys = np.full((h, w, D + 1), 0xffffffff, np.uint64)   # (one more column, so that a lone candidate has a partner)
    for dd in range(D):
        keys[:, :w - dd, dd] = (S[:, dd:, dd].astype(np.uint64) << np.uint64(16)) | np.uint64(dd)
    return left, _decide(keys, uniqueness)


def median3(p):
    h, w = p.shape
    out = np.zeros_like(p)
    if h >= 3 and w >= 3:
        stack = np.stack([p[1 + j:h - 1 + j, 1 + i:w - 1 + i] for j in (-1, 0, 1) for i in (-1, 0, 1)], -1)
        out[1:h - 1, 1:w - 1] = np.sort(stack, -1)[..., 4]
    return out


def consistency(med_left, med_right, left):
    h, w = med_left.shape
    out = med_left.astype(np.int64).copy()
    gw, gh = 16 * (w // 16), 16 * (h // 16)
    d = out[:gh, :gw]
    k = np.arange(gw)[None, :] - d
    inside = (k >= 0) & (k < w)
    rv = np.take_along_axis(med_right[:gh].astype(np.int64), np.clip(k, 0, w - 1), 1)
    bad = (np.asarray(left)[:gh, :gw] == 0) | (d <= 0) | (inside & (np.abs(rv - d) > 1))
    out[:gh, :gw] = np.where(bad, 0, d)
    return out.astype(np.uint8)


def depth(disp, baseline, focal):
    d = disp.astype(np.float64)
    with np.errstate(divide="ignore"):
        t = ((200.0 * np.float64(baseline)) * np.float64(focal)) / d
    t = np.where((disp == 0) | (t > 255) | (t < 0), 0.0, t)
    return np.trunc(t).astype(np.uint8)


def run(left, right, D=128, P1=10, P2=120, uniqueness=0.96, baseline=1.0, focal=1.0):
    """-> the dict of every plane msfm_sgm_fetch returns, by the names of metricsfm_amd._abi.SGM_FETCH (path_cost: [8][h][w][D]),
    and depth"""
    cl, cr = census(left), census(right)
    C = matching_cost(cl, cr, D)
    paths = [path_cost(C, r, P1, P2) for r in range(8)]
    S = sum(paths)
    raw_l, raw_r = winners(S, uniqueness)
    med_l, med_r = median3(raw_l), median3(raw_r)
    fin = consistency(med_l, med_r, left)
    return dict(census_left=cl, census_right=cr, path_cost=np.stack(paths).astype(np.uint8), raw_left=raw_l, raw_right=raw_r,
                median_left=med_l, median_right=med_r, disparity=fin, depth=depth(fin, baseline, focal), cost_max=int(np.max(paths)))
