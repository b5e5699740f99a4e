"""GPU: random-shape sweep of the conv engine (tools/conv_fuzz.py): forward with a random fused epilogue, input gradient and weight gradient in
the three arithmetics against float64 at shapes the model never uses (odd extents, channel counts that are no tile multiple, 1-pixel maps,
strides).  Unsupported configurations must be refused with an error, never answered with wrong values.  (600 cases: profiles/r04_conv_fuzz.txt.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_random_conv_shapes_match_float64_or_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_fuzz.py"), "--cases", "120", "--seed", "7"], capture_output=True, text=True,
                       timeout=550, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "FAILURES: 0" in r.stdout, tail
    # the only refusals are the documented vector-width requirements of the backward kernels
    for line in r.stdout.split("refused (RuntimeError) configurations:")[-1].splitlines():
        if " x " in line:
            assert "multiple of 4" in line or "multiples of 4" in line, line


# The route-stratified part of the sweep: each group of strata is drawn towards a route, confirmed with the library (ops.conv_route_info) and
# must have covered what tests/conv_ref.py::fuzz_coverage_problems lists -- the same conditions tests/test_conv_fuzz_plan.py checks on the
# generator alone, here on the comparisons that actually ran.  24 cases per stratum: the smallest counts for which the plan of seed 7 meets
# the conditions are 9 / 12 / 6 (winograd / reduced / fused); 24 leaves every stratum a random share beyond them.
PER_STRATUM = 24


def _run_group(group):
    from conv_ref import FUZZ_GROUPS, fuzz_coverage, fuzz_coverage_problems
    strata = FUZZ_GROUPS[group]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_fuzz.py"), "--strata", ",".join(strata), "--per-stratum", str(PER_STRATUM),
                        "--seed", "7"], capture_output=True, text=True, timeout=550, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    print(r.stdout[-6000:])
    assert r.returncode == 0, tail
    assert "FAILURES: 0" in r.stdout, tail
    bad = fuzz_coverage_problems(fuzz_coverage(r.stdout), strata, PER_STRATUM)
    assert not bad, bad
    # the only refusals are the documented vector-width requirements of the backward kernels
    for line in r.stdout.split("refused (RuntimeError) configurations:")[-1].splitlines():
        if " x " in line:
            assert "multiple of 4" in line or "multiples of 4" in line, line


@pytest.mark.timeout(600)
def test_winograd_routes_match_float64_at_every_tile_residue():
    """wino: forward, input gradient, weight gradient and the weight gradient from the forward's kept V, all confirmed Winograd, in f32, bf16x6
    and f16x3, for every H % 4 and W % 4, maps smaller than a tile and batches of 40..96 one-tile images.  wino_wgrad_only: the mixed route
    (forward direct, weight gradient Winograd) for each way a wide 3x3 conv falls off the forward route."""
    _run_group("winograd")


@pytest.mark.timeout(600)
def test_reduced_precision_routes_match_their_definitions():
    """f16: ABR_MATH_F16 against float64 on the mode's rounded operands (test_gpu_f16_math.py's bound); bf16_fallback: ABR_MATH_BF16 at channel
    counts that are no multiple of 64 runs in fp32 and meets fp32's tolerance"""
    _run_group("reduced")


@pytest.mark.timeout(600)
def test_fused_tail_and_fused_input_gradient_match_float64():
    """tail64: the fused bottleneck tail bit-equal to the two convs it replaces; dgrad_fused: the input gradient with the ReLU mask and / or
    a residual in its epilogue, ordinary and scattered"""
    _run_group("fused")
