"""The HIP bundle adjustment against the CPU oracle at the options, stopping rules and failure paths that no other GPU test
reaches: huber_delta, the LM-diagonal clamps, jacobi_scaling, min_relative_decrease, both radius bounds,
max_num_consecutive_invalid_steps, every termination of msfm_ba_run and invalid steps.

The oracle's own handling of each option set is pinned against SparseLM first (tests/test_oracle.py); the scenes, option
sets and the condition on the inputs live in tests/ba_option_cases.py.  Every comparison uses check_parity_strict
(tests/test_gpu_ba.py): cost 1e-9, parameters 1e-7, radius 1e-6, |gradient|_max and |step| 1e-5, rho and cost change 1e-5
(+ 1e-9 x cost), the step counters, initial and final cost.

Condition on the inputs, asserted on the oracle's rows before the GPU is looked at (ba_option_cases.decision_margins):
|rho - min_relative_decrease| >= 0.05 and |cost_change| >= 1e-6 x cost on every valid row; a tolerance that fires has its
tested quantity below half its bound, and above twice its bound on every earlier row.  Three departures from the recipes this
file was specified with, each because the recipe did not meet that condition in the oracle:
  cap-R runs 8 iterations, not 12 (the relative cost change of steps 9 - 12 is 7e-7 ... 1e-8);
  param-R has parameter_tolerance 1e-3, not 1e-2, and 2 recorded iterations, not 1 (|step| / |x| is 2.3e-2, 5.9e-3, 2.7e-4:
  at 1e-2 the firing step sits at 0.59 of its bound, at 1e-3 the third step at 0.27 and the second at 5.9);
  grad-J (gradient_tolerance 3e5 between |g| = 4.13e5 and 1.77e5) has margins of 1.37x and 1.69x only - no two consecutive
  |g| of that run are a factor 4 apart - so it is held to a factor 1.3 (10^4 x the 1e-5 the two solvers' |g| agree to), and
  grad-R-late (R, tolerance 1.5e3 between |g| = 3.9e3 and 5.0e2) is the same stop - behind an accepted step, the next
  linearisation already enqueued - with the full factor 2.

Per case: the oracle's termination, recorded rows, smallest decision margins (|rho - mrd|, |cost change| / cost), and the
largest deviation GPU vs oracle measured on an MI355X for cost (bar 1e-9), parameters (bar 1e-7) and rho (bar 1e-5):
  case                termination            rows  |rho-mrd|  |dcost|/c       cost    param      rho
  huber-O-0.25        NO_CONVERGENCE            7       1.75    0.00237   7.09e-13 1.66e-13 2.99e-12
  huber-O-4           NO_CONVERGENCE            7       1.49   0.000846   2.49e-13 2.21e-13 1.58e-12
  huber-O-1e6         NO_CONVERGENCE            7      0.409    3.1e-05   4.87e-13 3.31e-13 8.95e-11
  huber-G-0.25        NO_CONVERGENCE            7       1.75    0.00237   5.62e-13 2.31e-13 1.73e-12
  huber-G-4           NO_CONVERGENCE            7        1.5   0.000843   2.21e-13 5.15e-12 2.71e-11
  huber-J-0.25        NO_CONVERGENCE            7        1.4      0.603   1.05e-10 3.95e-14 1.06e-10
  huber-J-400         NO_CONVERGENCE            9      0.455       0.21   1.88e-10 9.28e-14 1.89e-10
  lmdiag-min10        NO_CONVERGENCE            7       1.09       0.15   4.24e-15 6.91e-15 2.24e-14
  lmdiag-max1e-4      NO_CONVERGENCE            7       1.69    0.00189   3.44e-13 4.81e-12 4.67e-12
  lmdiag-noscale      NO_CONVERGENCE            7       1.39      0.149   4.90e-15 2.85e-15 4.31e-14
  lmdiag-zero-weight  NO_CONVERGENCE            7       1.41      0.199   4.58e-15 6.10e-15 2.08e-14
  cap-R               NO_CONVERGENCE            9       1.13   2.69e-06   1.79e-11 1.71e-12 3.78e-09
  mrd-O               NO_CONVERGENCE            9       0.09   6.45e-06   4.87e-13 3.67e-13 9.84e-10
  mrd-J               NO_CONVERGENCE           13     0.0923     0.0409   2.32e-10 2.48e-13 2.32e-10
  minrad-R            MIN_RADIUS                1        inf        inf   9.59e-16 0.00e+00 0.00e+00
  minrad-J            MIN_RADIUS                2        376      0.994   1.39e-11 0.00e+00 1.40e-11
  grad-R              CONVERGENCE_GRADIENT      1        inf        inf   9.59e-16 0.00e+00 0.00e+00
  grad-R-late         CONVERGENCE_GRADIENT      5       1.13     0.0125   1.85e-11 2.05e-12 3.78e-12
  grad-J              CONVERGENCE_GRADIENT     11       1.29      0.167   2.32e-10 3.13e-13 2.32e-10
  param-R             CONVERGENCE_PARAMETER     3       1.72      0.859   1.85e-11 2.05e-12 1.42e-12
  func-R              CONVERGENCE_FUNCTION      4        1.2       0.43   1.85e-11 2.05e-12 3.78e-12
  fail-Z-5            FAILURE                   5        inf        inf   0.00e+00 0.00e+00 0.00e+00
  fail-Z-3            FAILURE                   3        inf        inf   0.00e+00 0.00e+00 0.00e+00
  fail-Z-1            FAILURE                   1        inf        inf   0.00e+00 0.00e+00 0.00e+00
  grad-Z              CONVERGENCE_GRADIENT      1        inf        inf   0.00e+00 0.00e+00 0.00e+00
  (inf: no valid step in the run.  Z: every figure is exactly 0.)
"""
import ctypes as C

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from tests import ba_option_cases as K
from tests.test_gpu_ba import check_parity_strict

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(oracle, name):
    """The oracle's run of a case: computed once, shared by every test that needs it, never written to again."""
    if name not in _REF:
        c = K.CASES[name]
        a = K.case_arrays(name)
        r = oracle.ba_solve(a, oracle.default_options(**c["opts"]))
        for x in (a.cam_pose, a.cam_model, a.point, r["iterations"]):
            x.setflags(write=False)
        _REF[name] = (r, a)
    return _REF[name]


def _gradient_factor(name):
    return 1.3 if name == "grad-J" else 2.0      # (see the module docstring)


def _gpu_vs_oracle(ctx, oracle, name):
    from metricsfm_amd import capi
    c = K.CASES[name]
    r_ref, a_ref = _reference(oracle, name)
    if name in K.EXPECT:
        assert (r_ref["termination"], r_ref["num_iterations"]) == K.EXPECT[name]
    m_rho, m_chg = K.decision_margins(r_ref, c["opts"], gradient_factor=_gradient_factor(name))   # the inputs first, from the oracle alone
    print("%s: oracle %s, %d rows, margins |rho - mrd| %.3g, |cost change| / cost %.3g"
          % (name, r_ref["termination"], len(r_ref["iterations"]), m_rho, m_chg))
    a_gpu = K.case_arrays(name)
    r_gpu = ctx.ba_solve(a_gpu, capi.default_options(**c["opts"]))
    check_parity_strict(r_gpu, r_ref, a_gpu, a_ref)
    return r_gpu, r_ref, a_gpu


def _assert_parameters_are_the_input(a, name):
    a0 = K.case_arrays(name)
    for f in ("cam_pose", "cam_model", "point"):
        np.testing.assert_array_equal(getattr(a, f), getattr(a0, f))


def _both_sides(states, select, delta, least=10):
    """At least `least` residual blocks above delta and as many below it, at iteration 0 or at the oracle's last iterate."""
    above = max(int((select(st) > delta).sum()) for st in states)
    below = max(int((select(st) < delta).sum()) for st in states)
    return above >= least and below >= least


@pytest.mark.parametrize("name", ["huber-O-0.25", "huber-O-4", "huber-O-1e6", "huber-G-0.25", "huber-G-4", "huber-J-0.25", "huber-J-400"])
def test_huber_delta(ctx, oracle, name):
    """huber_delta is read by k_point, the rows of frozen points (k_linearize), k_gps and k_tail; every other test hands them 1.
    Asserted on the inputs: residual blocks lie on both sides of the threshold - at iteration 0 where the start allows it
    (delta 4: 20 rows below; J at 400: frozen rows on both sides; the GPS blocks, whose weight is chosen for it), else at the
    oracle's last iterate (O starts with every row above 0.25 and ends with 600 below) - and none above it at 1e6.
    J at 0.25 keeps every row, the frozen ones included, on the outlier branch throughout: that is what it is for."""
    c = K.CASES[name]
    delta = c["opts"]["huber_delta"]
    _, a_ref = _reference(oracle, name)
    states = [K.row_norms(c["scene"]), K.row_norms(c["scene"], at=a_ref)]
    if delta == 1e6:
        assert all((st[0] < delta).all() for st in states)
    elif name == "huber-J-0.25":
        assert all((st[0] > delta).all() for st in states) and (~states[0][1]).sum() > 1000 and (~states[0][2]).sum() > 500
    else:
        assert _both_sides(states[:1] if delta >= 4.0 else states, lambda st: st[0], delta)
    if name == "huber-J-400":
        assert _both_sides(states[:1], lambda st: st[0][~st[2]], delta)      # rows of frozen points, at iteration 0
        assert _both_sides(states[:1], lambda st: st[0][~st[1]], delta)      # rows of frozen cameras
    if c["scene"] == "G":
        g = K.gps_rows("G", K.gps_weight_for(c["gps_delta"]))
        assert (g > 1.05 * delta).sum() >= 3 and (g < delta / 1.05).sum() >= 3, g      # GPS blocks on both sides, from the arrays
    _gpu_vs_oracle(ctx, oracle, name)


@pytest.mark.parametrize("name", ["lmdiag-min10", "lmdiag-max1e-4", "lmdiag-noscale", "lmdiag-zero-weight"])
def test_lm_diagonal_clamps_and_jacobi_scaling(ctx, oracle, name):
    """min_lm_diagonal / max_lm_diagonal in the assemble kernels and k_point, at radius 1 where the damping shows; jacobi_scaling
    off together with clamps that bind (alone it moves rho in the 4th digit only: LM with Marquardt's diagonal is scale
    invariant).  An option that does not bind tests nothing: the oracle's costs must leave its default-option run by > 1e-3."""
    r_ref, _ = _reference(oracle, name)
    if name != "lmdiag-zero-weight":
        r_def, _ = _reference(oracle, "lmdiag-default")
        assert (np.abs(r_ref["iterations"]["cost"] / r_def["iterations"]["cost"] - 1.0) > 1e-3).any()
    else:
        a = K.case_arrays(name)
        assert (a.pt_weight[::7] == 0).all() and (a.pt_weight > 0).sum() > 1000
    _gpu_vs_oracle(ctx, oracle, name)


def test_radius_cap(ctx, oracle):
    """Every step of R is accepted and triples the radius: max_trust_region_radius = 2e4 binds from the first step on."""
    r_gpu, r_ref, _ = _gpu_vs_oracle(ctx, oracle, "cap-R")
    want = np.array([1e4] + [2e4] * 8)
    np.testing.assert_array_equal(r_ref["iterations"]["trust_region_radius"], want)
    np.testing.assert_array_equal(r_gpu["iterations"]["trust_region_radius"], want)
    assert r_ref["iterations"]["step_is_successful"].all()


@pytest.mark.parametrize("name", ["mrd-O", "mrd-J"])
def test_min_relative_decrease(ctx, oracle, name):
    """Steps that the default 1e-3 would accept are rejected: rho between the two thresholds, 0.05 away from either."""
    mrd = K.CASES[name]["opts"]["min_relative_decrease"]
    it = _reference(oracle, name)[0]["iterations"]
    turned = (it["step_is_successful"] == 0) & (it["relative_decrease"] > K.DEFAULT_MIN_RELATIVE_DECREASE + 0.05) & (it["relative_decrease"] < mrd - 0.05)
    assert turned[1:].sum() >= (2 if name == "mrd-O" else 1) and (it["step_is_successful"][1:] == 1).sum() >= 3
    if name == "mrd-J":
        assert turned[-1]         # the last step, rho 0.808
    _gpu_vs_oracle(ctx, oracle, name)


@pytest.mark.parametrize("name", ["minrad-R", "minrad-J"])
def test_min_radius(ctx, oracle, name):
    """MIN_RADIUS before any step (initial radius = minimum: no step is enqueued at all) and behind the first rejection
    (1e4 / 2 < 6e3).  Either way the parameters are the input's, bit for bit."""
    r_gpu, r_ref, a_gpu = _gpu_vs_oracle(ctx, oracle, name)
    assert r_gpu["termination"] == "MIN_RADIUS"
    _assert_parameters_are_the_input(a_gpu, name)
    if name == "minrad-J":
        np.testing.assert_array_equal(r_gpu["iterations"]["trust_region_radius"], [1e4, 5e3])


@pytest.mark.parametrize("name", ["grad-R", "grad-R-late", "grad-J"])
def test_gradient_tolerance(ctx, oracle, name):
    """CONVERGENCE_GRADIENT with a non-empty problem.  At iteration 0 the step enqueued with the first reduced system - and the
    linearisation enqueued behind it - are discarded: parameters bit-identical to the input proves they wrote the candidate
    buffers only.  Later it stops behind an accepted step, with the launch-ahead of the following step in flight."""
    r_gpu, r_ref, a_gpu = _gpu_vs_oracle(ctx, oracle, name)
    assert r_gpu["termination"] == "CONVERGENCE_GRADIENT"
    if name == "grad-R":
        _assert_parameters_are_the_input(a_gpu, name)
    else:
        assert r_gpu["iterations"]["step_is_successful"][-1] == 1 and r_gpu["num_iterations"] >= 4


@pytest.mark.parametrize("name", ["param-R", "func-R"])
def test_parameter_and_function_tolerance(ctx, oracle, name):
    """CONVERGENCE_PARAMETER / CONVERGENCE_FUNCTION: the device's verdict on a step that is never recorded."""
    ratio = K.firing_margin(oracle.ba_solve, oracle.default_options, name)
    print("%s: tested quantity / bound per step %s" % (name, np.array2string(ratio, precision=3)))
    r_gpu, _, _ = _gpu_vs_oracle(ctx, oracle, name)
    assert r_gpu["termination"] == K.EXPECT[name][0]


@pytest.mark.parametrize("name", ["fail-Z-5", "fail-Z-3", "fail-Z-1", "grad-Z"])
def test_invalid_steps_and_failure(ctx, oracle, name):
    """Every weight 0: residuals, Jacobian and gradient are exactly zero, every diagonal clamps to min_lm_diagonal, the
    factorisations succeed, the step is exactly zero and model_cost_change == 0 makes it invalid - no non-finite number and
    no indefinite system anywhere (the kernels' waits are bounded and depend on the launch structure only, which is R's).
    The radius is divided by 2, 4, 8, 16; the max_num_consecutive_invalid_steps-th invalid step ends the run, unrecorded."""
    a0 = K.case_arrays(name)
    assert (a0.pt_weight == 0).all()
    r_gpu, r_ref, a_gpu = _gpu_vs_oracle(ctx, oracle, name)
    n = K.EXPECT[name][1]
    it = r_gpu["iterations"]
    assert r_gpu["termination"] == K.EXPECT[name][0] and r_gpu["num_iterations"] == n
    np.testing.assert_array_equal(it["step_is_valid"], [1, 0, 0, 0, 0][:n + 1])
    np.testing.assert_array_equal(it["trust_region_radius"], [1e4, 5e3, 1.25e3, 156.25, 9.765625][:n + 1])
    assert (it["cost"] == 0).all() and r_gpu["final_cost"] == 0 and r_gpu["num_unsuccessful_steps"] == n
    _assert_parameters_are_the_input(a_gpu, name)


def _rows_equal(x, y):
    assert x["termination"] == y["termination"] and x["num_iterations"] == y["num_iterations"]
    assert x["num_successful_steps"] == y["num_successful_steps"] and x["num_unsuccessful_steps"] == y["num_unsuccessful_steps"]
    assert x["iterations"].tobytes() == y["iterations"].tobytes()
    assert x["initial_cost"] == y["initial_cost"] and x["final_cost"] == y["final_cost"]


@pytest.mark.parametrize("name", ["minrad-R", "minrad-J", "grad-R", "grad-R-late", "grad-J", "param-R", "func-R", "fail-Z-3"])
def test_every_termination_in_both_launch_orders_and_on_a_resident_problem(ctx, monkeypatch, name):
    """MSFM_SPEC=0 (the next linearisation enqueued after the read-back) and 1 (ahead of it) give bitwise the same rows and
    parameters at every termination.  On a resident problem nothing enqueued ahead of a stop survives it: a second run
    (default options, 3 iterations) equals, bitwise, a fresh problem given the first run's parameters and run the same way."""
    from metricsfm_amd import capi
    opts = K.CASES[name]["opts"]
    out = []
    for spec in ("0", "1"):
        monkeypatch.setenv("MSFM_SPEC", spec)
        a = K.case_arrays(name)
        out.append((ctx.ba_solve(a, capi.default_options(**opts)), a))
    monkeypatch.delenv("MSFM_SPEC")
    (r0, a0), (r1, a1) = out
    assert r0["termination"] == K.EXPECT[name][0]
    _rows_equal(r0, r1)
    for f in ("cam_pose", "cam_model", "point"):
        np.testing.assert_array_equal(getattr(a0, f), getattr(a1, f))
    second = capi.default_options(max_num_iterations=3)
    ba = ctx.ba(K.case_arrays(name))
    ra = ba.run(capi.default_options(**opts))
    params = ba.download()
    rb = ba.run(second)
    after = ba.download()
    ba.close()
    _rows_equal(ra, r1)
    for x, f in zip(params, ("cam_pose", "cam_model", "point")):
        np.testing.assert_array_equal(x, getattr(a1, f))
    fresh = ctx.ba(K.case_arrays(name))
    fresh.upload(*params)
    rf = fresh.run(second)
    after_fresh = fresh.download()
    fresh.close()
    _rows_equal(rb, rf)
    for x, y in zip(after, after_fresh):
        np.testing.assert_array_equal(x, y)


def test_row_capacity(ctx):
    """iterations_capacity = 3 on a run of 8 iterations: the first 3 rows are those of a full-capacity run, num_iterations is
    still 8 and nothing is written behind the third row (the buffer is longer than the library is told, and holds a pattern)."""
    from metricsfm_amd import capi
    opts = capi.default_options(**K.CASES["cap-R"]["opts"])
    full = ctx.ba_solve(K.case_arrays("cap-R"), opts)
    assert full["num_iterations"] == 8 and len(full["iterations"]) == 9
    buf = A.SummaryBuf(16)
    buf.rows.view(np.uint8)[:] = 0xA5
    buf.struct.iterations_capacity = 3
    a = K.case_arrays("cap-R")
    ctx.check(capi.lib().msfm_ba_solve(ctx._h, C.byref(a.struct), C.byref(opts), C.byref(buf.struct)))
    s = buf.struct
    assert s.num_iterations == 8 and s.num_successful_steps == full["num_successful_steps"] and s.final_cost == full["final_cost"]
    assert buf.rows[:3].tobytes() == full["iterations"][:3].tobytes()
    assert (buf.rows[3:].view(np.uint8) == 0xA5).all()
