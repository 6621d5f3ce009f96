"""The cases of the dense-stereo tests and the C++ restatement (tests/sgm_ref.cpp) run on them once per process: built with g++
into a temporary directory, fed one binary file, its planes read back read-only and shared by every test that needs them."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (("census_left", np.uint32), ("census_right", np.uint32), ("path_cost", np.uint8), ("raw_left", np.uint16), ("raw_right", np.uint16),
          ("median_left", np.uint16), ("median_right", np.uint16), ("disparity", np.uint8), ("depth", np.uint8))
DEFAULTS = dict(P1=10, P2=120, uniqueness=0.96)
BASELINE, FOCAL = 0.05, 300.0   # 200 * 0.05 * 300 = 3000: depth 0 for disparities below 12 (t > 255), 250 and less from there on


def launch_constants():
    """SGM_LANE_DISP, SGM_PATH_THREADS, SGM_WTA_TILE as metricsfm_amd/csrc/sgm_args.h defines them."""
    with open(os.path.join(ROOT, "metricsfm_amd", "csrc", "sgm_args.h")) as fh:
        text = fh.read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % n, text).group(1)) for n in ("SGM_LANE_DISP", "SGM_PATH_THREADS", "SGM_WTA_TILE"))


def path_groups(D):
    """Lane groups (columns, diagonals or rows) per workgroup of the path kernels at D disparities."""
    lane_disp, threads, _ = launch_constants()
    return threads // (D // lane_disp)


# name -> (D, w, h, seed): the table of the issue, then per D one case that is one pixel larger, in both dimensions, than a
# multiple of the path kernels' groups per workgroup (SGM_PATH_THREADS / (D / SGM_LANE_DISP): 32 at D = 64, 16 at D = 128; the
# width is the smallest such number that is not below D)
CASES = {
    "odd64": (64, 83, 37, 1),
    "flat64": (64, 64, 5, 2),
    "onerow64": (64, 64, 7, 3),
    "odd128": (128, 150, 21, 4),
    "grid128": (128, 272, 64, 5),
    "groups64": (64, 2 * path_groups(64) + 1, path_groups(64) + 1, 6),
    "groups128": (128, 8 * path_groups(128) + 1, path_groups(128) + 1, 7),
}
SMALLEST = ("flat64", "onerow64")


def texture(w, h, seed):
    """Random texture with some structure larger than a pixel, uint8, values 1 .. 255."""
    rng = np.random.default_rng(seed)
    fine = rng.integers(1, 256, (h, w)).astype(np.float64)
    coarse = np.kron(rng.integers(1, 256, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4)))[:h, :w]
    return np.clip(np.rint(0.6 * fine + 0.4 * coarse), 1, 255).astype(np.uint8)


def planted_pair(w, h, seed, d_top, d_bottom, noise=0.0):
    """-> (left, right, planted [h][w]): left(x, y) = right(x - d, y) with d = d_top in the upper half of the rows and d_bottom in
    the lower; the left columns that have no partner are texture of their own."""
    rng = np.random.default_rng(seed + 500)
    right = texture(w, h, seed)
    left = texture(w, h, seed + 250)
    planted = np.zeros((h, w), np.int32)
    half = h // 2
    for rows, d in ((slice(0, half), d_top), (slice(half, h), d_bottom)):
        left[rows, d:] = right[rows, :w - d]
        planted[rows] = d
    if noise:
        left = np.clip(np.rint(left + rng.normal(0, noise, left.shape)), 0, 255).astype(np.uint8)
        right = np.clip(np.rint(right + rng.normal(0, noise, right.shape)), 0, 255).astype(np.uint8)
    return left, right, planted


@functools.lru_cache(maxsize=None)
def case_pair(name, variant=0):
    """The pair of a case: seeded texture with two planted disparities, noise, a zero-valued patch in the left image and a flat
    patch in both.  variant: another seed for the same shape."""
    D, w, h, seed = CASES[name]
    left, right, _ = planted_pair(w, h, seed + 31 * variant, min(D // 8, w // 4), min(D // 3, w // 3), noise=2.0)
    left, right = left.copy(), right.copy()
    left[h // 3:h // 3 + 3, w // 2:w // 2 + 9] = 0
    y0, x0 = max(h // 2 - 2, 0), w // 5
    left[y0:y0 + 6, x0:x0 + 14] = 90
    right[y0:y0 + 6, x0:x0 + 14] = 90
    for a in (left, right):
        a.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def ref_exe():
    exe = os.path.join(tempfile.mkdtemp(prefix="sgm_ref_"), "sgm_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "sgm_ref.cpp"), "-o", exe])
    return exe


def run_ref_cpp(left, right, D, P1=10, P2=120, uniqueness=0.96, baseline=BASELINE, focal=FOCAL, volumes=True):
    """-> dict of the planes in PLANES (path_cost [8][h][w][D], absent without `volumes`) and seconds, arrays read-only"""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    h, w = left.shape
    tmp = tempfile.mkdtemp(prefix="sgm_io_")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        np.array([w, h, D, P1, P2, 0 if volumes else 1], np.int32).tofile(fh)
        np.array([uniqueness], np.float32).tofile(fh)
        np.array([baseline, focal], np.float64).tofile(fh)
        left.tofile(fh)
        right.tofile(fh)
    try:
        out = subprocess.run([ref_exe(), fin, fout], capture_output=True, text=True)
        assert out.returncode == 0 and "sgm_ref ok" in out.stdout, out.stdout + out.stderr
        got = {}
        with open(fout, "rb") as fh:
            for name, dt in PLANES:
                if name == "path_cost":
                    if volumes:
                        got[name] = np.fromfile(fh, dt, 8 * h * w * D).reshape(8, h, w, D)
                    continue
                got[name] = np.fromfile(fh, dt, h * w).reshape(h, w)
    finally:
        for p in (fin, fout):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
    for a in got.values():
        a.setflags(write=False)
    got["seconds"] = float(out.stdout.split(",")[1].split()[0])
    return got


@functools.lru_cache(maxsize=None)
def expected(name, P1=10, P2=120, uniqueness=0.96, variant=0):
    """The restatement's planes for a case and a parameter set, computed once and shared."""
    left, right = case_pair(name, variant)
    return run_ref_cpp(left, right, CASES[name][0], P1, P2, uniqueness)
