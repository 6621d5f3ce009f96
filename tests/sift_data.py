"""Seeded synthetic images and frame lists for the SIFT tests, and the C++ restatement (tests/sift_ref.cpp) run on them once per
process.  The host numbers - taps, window table, per-frame records - come from tests/sift_ref.py, which computes them with the C
library as metricsfm_amd/csrc/sift_args.h does."""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from tests import sift_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def image(w, h, seed, const_patch=None):
    """Gaussian blobs of several widths, a ramp and uniform noise, uint8 [h][w]; const_patch = (x0, y0, x1, y1) is made one value."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 40.0 + 60.0 * xx / w + 30.0 * yy / h
    for width in (1.5, 3.0, 6.0, 11.0):
        for _ in range(6):
            cx, cy, a = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(-70, 90)
            v += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * width * width))
    v += rng.uniform(-6, 6, (h, w))
    img = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if const_patch is not None:
        x0, y0, x1, y1 = const_patch
        img[y0:y1, x0:x1] = 117
    return img


def sigma_for(S, o, i_s):
    """A sigma that the frame-to-level rule sends to (o, i_s)."""
    return 1.6 * math.pow(2.0, 1.0 / S) * 2.0 ** (o + i_s / S)


# name -> (w, h, stride, O, S, seed, constant patch)
CASES = {
    "a": (96, 80, 96, 3, 5, 11, (50, 34, 96, 80)),
    "b": (75, 61, 75, 4, 5, 12, None),
    "c": (130, 70, 144, 3, 3, 13, None),
}


def case_image(name):
    w, h, stride, O, S, seed, patch = CASES[name]
    return image(w, h, seed, patch)


def case_frames(name, ang):
    """The frame list [n][4] of a case; ang[o][s]: the restated angle planes (for the frames whose th lands at 0 and at 2 pi).
    -> (frames, dict of named indices)"""
    w, h, stride, O, S, seed, patch = CASES[name]
    rng = np.random.default_rng(seed + 100)
    fr, idx = [], {}
    for o in range(O):                       # interior frames at every (o, is), two each
        for i_s in range(S):
            for _ in range(2):
                fr.append((rng.uniform(0.3 * w, 0.7 * w), rng.uniform(0.3 * h, 0.7 * h), sigma_for(S, o, i_s), rng.uniform(-7, 7)))
    idx["clamp_low"] = len(fr)
    fr.append((0.5 * w, 0.5 * h, 0.05, 0.3))             # far below sigma0 / 2
    idx["clamp_high"] = len(fr)
    fr.append((0.5 * w, 0.5 * h, 1.0e4, 0.3))            # far above the top octave
    for x, y in ((2.2, 0.5 * h), (w - 2.6, 0.5 * h), (0.5 * w, 1.7), (0.5 * w, h - 2.8), (1.0, 1.0), (w - 1.0, h - 2.0)):   # cut by each border
        fr.append((x, y, 2.0, 1.0))
    idx["outside"] = list(range(len(fr), len(fr) + 6))
    for x, y in ((-5.0, 0.5 * h), (w + 10.0, 0.5 * w), (0.5 * w, -3.0), (0.5 * w, h - 0.4), (0.5 * w, h - 1.2), (float(w), 3.0)):
        fr.append((x, y, 2.0, 0.0))
    px, py = int(0.4 * w), int(0.45 * h)
    for th in (0.0, math.pi / 2, math.pi, 3 * math.pi / 2, 1.234, -5.0):
        fr.append((px + 0.25, py - 0.25, 1.9, th))
    # th within one ulp of 0 and of 2 pi: theta = the angle at the frame's centre pixel on level (0, 0), and its neighbours
    a = F32(ang[0][0][py, px])
    for th in (a, np.nextafter(a, F32(7)), np.nextafter(a, F32(-1))):
        fr.append((float(px), float(py), 0.9, float(th)))
    idx["twins"] = (len(fr), len(fr) + 1)
    fr += [(0.61 * w, 0.37 * h, 3.3, 2.2)] * 2
    if patch is not None:
        idx["constant"] = len(fr)
        fr.append((74.0, 58.0, 0.8, 0.7))
    return np.array(fr, np.float64).astype(F32), idx


@functools.lru_cache(maxsize=None)
def ref_exe(flags=("-O2",)):
    """tests/sift_ref.cpp built once per process (and per flag set)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="sift_ref_"), "sift_ref")
    subprocess.check_call(["g++", *flags, "-ffp-contract=off", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "sift_ref.cpp"), "-o", exe])
    return exe


def run_ref_cpp(img, O, S, frames, exe=None):
    """-> dict(gss[o][s + 1], mod[o][s], ang[o][s], rows {0, 1: [n][128]}, seconds (scale space, descriptors), records)"""
    exe = exe or ref_exe()
    taps, T = R.host_numbers(S)
    rec = R.frame_records(frames, O, S)
    h, w = img.shape
    tmp = tempfile.mkdtemp(prefix="sift_io_")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        np.array([w, h, O, S, len(rec)], np.int32).tofile(fh)
        np.ascontiguousarray(img, np.uint8).tofile(fh)
        for g in taps:
            np.array([len(g)], np.int32).tofile(fh)
            g.tofile(fh)
        T.tofile(fh)
        rec.tofile(fh)
    try:
        out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert out.returncode == 0 and "sift_ref ok" in out.stdout, out.stdout + out.stderr
        secs = [float(p.split()[0]) for p in out.stdout.split(",")[1:3]]
        gss, mod, ang = [], [], []
        with open(fout, "rb") as fh:
            for o in range(O):
                wo, ho = w >> o, h >> o
                plane = lambda: np.fromfile(fh, F32, wo * ho).reshape(ho, wo)   # noqa: E731
                gss.append([plane() for _ in range(S + 3)])
                m, a = [], []
                for _ in range(S):
                    m.append(plane())
                    a.append(plane())
                mod.append(m)
                ang.append(a)
            rows = {q: np.fromfile(fh, F32, len(rec) * 128).reshape(len(rec), 128) for q in (0, 1)}
    finally:
        for p in (fin, fout):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
    return dict(gss=gss, mod=mod, ang=ang, rows=rows, seconds=secs, records=rec)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's answer for a case, computed once and shared: dict of run_ref_cpp plus img, frames, idx."""
    w, h, stride, O, S, seed, patch = CASES[name]
    img = case_image(name)
    planes = run_ref_cpp(img, O, S, np.zeros((0, 4), F32))
    frames, idx = case_frames(name, planes["ang"])
    out = run_ref_cpp(img, O, S, frames)
    out.update(img=img, frames=frames, idx=idx)
    for v in out["rows"].values():
        v.setflags(write=False)
    return out
