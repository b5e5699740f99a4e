"""CPU: the random conv sweep (tools/conv_fuzz.py) reaches every route it claims to.  `--plan` draws the cases of the seed the GPU tests use,
asks the library which route each takes (abr_conv_route_info, host only) and prints the counts; the coverage conditions are the ones
tests/test_gpu_conv_fuzz.py asserts on the comparisons that ran.  Fails when a stratum is removed, a residue class is lost, or
abr::conv_route changes so that a stratum lands on other kernels than it was drawn for."""
import os
import subprocess
import sys

import pytest

from conv_ref import FUZZ_GROUPS, fuzz_coverage, fuzz_coverage_problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_STRATUM = 24      # tests/test_gpu_conv_fuzz.py::PER_STRATUM


def _plan(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_fuzz.py"), "--plan", "--seed", "7"] + list(args), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "FAILURES: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return fuzz_coverage(r.stdout)


def test_gpu_tests_per_stratum_is_this_files():
    src = open(os.path.join(ROOT, "tests", "test_gpu_conv_fuzz.py")).read()
    assert "PER_STRATUM = %d\n" % PER_STRATUM in src


@pytest.mark.parametrize("group", sorted(FUZZ_GROUPS))
def test_planned_strata_reach_their_routes(group):
    strata = FUZZ_GROUPS[group]
    cov = _plan("--strata", ",".join(strata), "--per-stratum", str(PER_STRATUM))
    assert sorted(cov) == sorted(strata)
    bad = fuzz_coverage_problems(cov, strata, PER_STRATUM, ran=False)
    assert not bad, bad


def test_a_lost_residue_or_a_lost_stratum_is_noticed():
    """the checker itself: drop one count from a good plan and it must say so"""
    strata = FUZZ_GROUPS["winograd"]
    cov = _plan("--strata", ",".join(strata), "--per-stratum", str(PER_STRATUM))
    del cov["wino"]["features"]["f16x3"]["wgrad_kept_v"]["W%4=1"]
    assert fuzz_coverage_problems(cov, strata, PER_STRATUM, ran=False) == ["wino: no confirmed-Winograd f16x3 wgrad_kept_v with W%4=1"]
    del cov["wino_wgrad_only"]
    assert "stratum wino_wgrad_only did not run" in fuzz_coverage_problems(cov, strata, PER_STRATUM, ran=False)


def test_blind_draw_is_the_sweeps_first_version():
    """stratum `any` keeps its generator: the first cases of seed 7 are the ones every earlier log of the sweep holds, and the blind draw
    rarely leaves the direct kernels (which is why the other strata exist)"""
    cov = _plan("--cases", "120")
    assert sorted(cov) == ["any"] and cov["any"]["cases"] == 120
    r = cov["any"]["routes"]["f32"]
    assert r.get("fwd/wino", 0) <= 6 and r["fwd/direct"] >= 110, r
