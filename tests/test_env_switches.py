"""Every ABR_* environment variable the package reads is a switch someone chose to keep: the set read by the sources equals the list
below, and DESIGN.md §7 documents each of them.  A new switch has to be added to both on purpose."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = {
    # library (abr_iod_amd/csrc)
    "ABR_IGEMM_FC_SPLIT", "ABR_IGEMM_SPLIT", "ABR_X6_NGROUP", "ABR_WINOGRAD_MIN_C", "ABR_WINOGRAD_WGRAD", "ABR_WINO_CACHE_MB",
    # Python package
    "ABR_ALLREDUCE_BACKEND", "ABR_ALLREDUCE_OVERLAP", "ABR_BF16_SCOPE", "ABR_BLOCK_PLANS", "ABR_CONV_MATH", "ABR_EARLY_PREFETCH",
    "ABR_EARLY_SECOND_PASS", "ABR_EVAL_GUARD", "ABR_H3_MAX_SMALL_FRACTION", "ABR_H3_STATS_EVERY", "ABR_H3_TAGS", "ABR_IOD_HIP_LIB",
    "ABR_JOINT_ROI", "ABR_PIPELINE_SOURCE", "ABR_PIPELINE_TARGET_FROZEN", "ABR_PROPOSAL_STREAM", "ABR_SHARE_FROZEN_PREFIX",
    "ABR_SOURCE_HEAD_STREAM", "ABR_SOURCE_OVERLAP", "ABR_SOURCE_STREAM", "ABR_STEP_MARKS", "ABR_WEIGHT_PREP_STREAM", "ABR_WGRAD_STREAM",
    "ABR_WGRAD_STREAMS", "ABR_WINOGRAD_KEEP_V", "ABR_X6_STRICT",
}

# getenv("ABR_X"), os.getenv("ABR_X"), os.environ.get("ABR_X"), os.environ["ABR_X"]
_READ = re.compile(r"""(?:getenv\s*\(|environ\s*(?:\.get\s*\(|\[))\s*["'](ABR_[A-Z0-9_]+)["']""")


def _sources():
    pkg = os.path.join(ROOT, "abr_iod_amd")
    return (sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)) + sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")))
            + sorted(glob.glob(os.path.join(pkg, "csrc", "*.h"))))


def _read_switches():
    found = {}
    for path in _sources():
        with open(path, encoding="utf-8") as f:
            for name in _READ.findall(f.read()):
                found.setdefault(name, os.path.relpath(path, ROOT))
    return found


def test_pattern_sees_every_form_of_read():
    src = '''getenv("ABR_A") os.getenv('ABR_B') os.environ.get("ABR_C", "1") os.environ["ABR_D"] environ.get( "ABR_E")'''
    assert set(_READ.findall(src)) == {"ABR_A", "ABR_B", "ABR_C", "ABR_D", "ABR_E"}


def test_switches_read_by_the_sources_are_the_listed_ones():
    found = _read_switches()
    unlisted = {k: v for k, v in found.items() if k not in SWITCHES}
    assert not unlisted, "switches read but not listed here (and in DESIGN.md §7): {}".format(unlisted)
    assert not SWITCHES - set(found), "listed switches no source reads any more: {}".format(sorted(SWITCHES - set(found)))


def test_every_switch_is_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        design = f.read()
    missing = sorted(n for n in SWITCHES if not re.search(r"\b{}\b".format(n), design))
    assert not missing, "switches missing from DESIGN.md: {}".format(missing)
