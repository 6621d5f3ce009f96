"""The cases of the SIFT detector tests and the C++ restatement (tests/siftdetect_ref.cpp) run on them once per process and per
threshold pair.  The three cases of tests/sift_data.py, and one image wide enough that a level spans three 256-pixel workgroups
of the extremum kernel in x and seventeen in y, and that its extremum masks (1300 words per level of octave 0) cross the
1024-word blocks of the scan.  The planes the restatement reads are the ones tests/sift_ref.cpp made."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests import sift_data as D
from tests import sift_ref as R

ROOT = D.ROOT
F32 = np.float32
STATS = ("candidates", "rejected_peak", "rejected_edge", "rejected_negative", "rejected_offset", "rejected_bounds", "keypoints", "n_found",
         "angles_0", "angles_1", "angles_2", "angles_3", "angles_4", "moved", "unconverged", "host_waits", "h2d_bytes", "d2h_bytes")
RAW_DT = np.dtype([("o", np.int32), ("ix", np.int32), ("iy", np.int32), ("is", np.int32), ("xn", F32), ("yn", F32), ("sn", F32),
                   ("flags", np.int32)])
KP_STATUS, KP_MOVED, KP_UNCONVERGED = 15, 16, 32

# name -> (w, h, stride, O, S, seed, constant patch), as sift_data.CASES
CASES = dict(D.CASES)
CASES["d"] = (600, 130, 608, 3, 3, 14, None)


def wide_image(w, h, seed):
    """sift_data.image plus what the detector's rules need to meet: many small blobs, down to widths below the first level's
    scale, and blobs beside the left and the right border."""
    rng = np.random.default_rng(seed + 1000)
    v = D.image(w, h, seed).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    spots = [(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.7, 3.0), rng.uniform(-60, 60)) for _ in range(160)]
    for cx, cy, wd, a in spots:
        v += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * wd * wd))
    # a flat strip along the left and the right border with blobs one and a half to two pixels inside the border.  The round
    # dark ones are flat-topped by the clip to 0: their extrema lie on the columns 1 and w - 2 and refine to within a hair of
    # the border.  The tilted ones (found by a search over such blobs on the restatement) couple x with y and scale: one refines
    # to xn < 0, one to sn < -1.
    v[:, :16] = 60.0
    v[:, w - 16:] = 60.0
    for y, cx, wd in ((18.0, 1.5, 2.0), (44.0, 2.0, 2.5), (118.0, 2.0, 2.5)):
        for bx, by in ((cx, y), (w - 1.0 - cx, y + 4.0)):
            v -= 100.0 * np.exp(-((xx - bx) ** 2 + (yy - by) ** 2) / (2 * wd * wd))
    for y, cx, s1, s2, th, a in ((70.0, 2.17, 2.78, 2.15, 1.15, -100.0), (94.0, 2.05, 2.61, 2.12, 2.15, -60.0)):
        c, s = np.cos(th), np.sin(th)
        p, q = (xx - cx) * c + (yy - y) * s, -(xx - cx) * s + (yy - y) * c
        v += a * np.exp(-(p * p / (2 * s1 * s1) + q * q / (2 * s2 * s2)))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_image(name):
    w, h, stride, O, S, seed, patch = CASES[name]
    return wide_image(w, h, seed) if name == "d" else D.image(w, h, seed, patch)


def blob_image(w=64, h=64, cx=32, cy=32, width=3.0):
    """One symmetric Gaussian blob on a flat ground, centred on a pixel: symmetric under both reflections about (cx, cy)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.rint(40.0 + 180.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * width * width))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ref_exe():
    exe = os.path.join(tempfile.mkdtemp(prefix="siftdetect_ref_"), "siftdetect_ref")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "siftdetect_ref.cpp"), "-o", exe])
    return exe


def run_detect_cpp(planes, w, h, O, S, peak_thresh=0.0, edge_thresh=10.0):
    """planes: the dict of sift_data.run_ref_cpp.  -> dict(stats, cells [n][4] (o, s, y, x), raw (RAW_DT), vals [n], frames [n_found][4], seconds)"""
    tmp = tempfile.mkdtemp(prefix="siftdetect_io_")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        np.array([w, h, O, S], np.int32).tofile(fh)
        np.array([peak_thresh, edge_thresh], F32).tofile(fh)
        R.host_numbers(S)[1].tofile(fh)
        for o in range(O):
            for p in planes["gss"][o]:
                p.tofile(fh)
            for s in range(S):
                planes["mod"][o][s].tofile(fh)
                planes["ang"][o][s].tofile(fh)
    try:
        out = subprocess.run([ref_exe(), fin, fout], capture_output=True, text=True)
        assert out.returncode == 0 and "siftdetect_ref ok" in out.stdout, out.stdout + out.stderr
        with open(fout, "rb") as fh:
            stats = np.fromfile(fh, np.int64, len(STATS))
            n = int(np.fromfile(fh, np.int64, 1)[0])
            cells = np.fromfile(fh, np.int32, 4 * n).reshape(n, 4)
            raw = np.fromfile(fh, RAW_DT, n)
            vals = np.fromfile(fh, F32, n)
            frames = np.fromfile(fh, F32).reshape(-1, 4)
    finally:
        for p in (fin, fout):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
    for a in (cells, raw, vals, frames):
        a.setflags(write=False)
    return dict(stats=dict(zip(STATS, (int(v) for v in stats))), cells=cells, raw=raw, vals=vals, frames=frames,
                seconds=float(out.stdout.split(",")[1].split()[0]))


@functools.lru_cache(maxsize=None)
def planes_of(name):
    w, h, stride, O, S, seed, patch = CASES[name]
    return D.expected(name) if name in D.CASES else D.run_ref_cpp(case_image(name), O, S, np.zeros((0, 4), F32))


@functools.lru_cache(maxsize=None)
def expected(name, peak_thresh=0.0, edge_thresh=10.0):
    """The restatement's answer for a case and a threshold pair, computed once and shared."""
    w, h, stride, O, S, seed, patch = CASES[name]
    return run_detect_cpp(planes_of(name), w, h, O, S, peak_thresh, edge_thresh)


def counters(stats):
    """The counters of a stats dict that the restatement also makes (everything but the bytes each way)."""
    return {k: v for k, v in stats.items() if not k.endswith("_bytes")}
