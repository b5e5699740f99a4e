"""CPU: the conv output-word rule (ops.conv_out_emits before the launch, ops.conv_out_done after it) row by row.

Under the f16x3 / f16 arithmetics a conv's epilogue may write the amax word of its result only where the pixels it writes are all the
tensor's non-zero pixels; a tensor tagged with a word that does not bound it gives silently wrong scales.  The expected values below are
conv_forward's, read off its code before the rule was shared, and written out as a table.  CPU tensors stand in for `out` and `residual`: the
rule looks at object identity, data_ptr() and the `_abr_scatter` mark only; nothing is launched."""
import pytest
import torch


def _t():
    return torch.zeros(1, 4, 4, 8)


def _case(kind, mark):
    """-> (out, residual) of a row: kind = fresh | residual (out is residual) | view (residual = another object over out's bytes) |
    other (a residual of its own) | none (no residual); mark = out's _abr_scatter: None | match | stale (another data_ptr) | (sh, sw)"""
    if kind == "fresh":
        return None, _t()
    out = _t()
    if mark == "match":
        out._abr_scatter = (out.data_ptr(), 2, 2)
    elif mark == "stale":
        out._abr_scatter = (out.data_ptr() + 64, 2, 2)
    elif mark is not None:
        out._abr_scatter = (out.data_ptr(),) + mark
    residual = {"residual": out, "view": out.view(1, 4, 4, 8), "other": _t(), "none": None}[kind]
    return out, residual


# (out, mark on out, (sh, sw) of the conv, emits, afterwards: tag | drop | none (a fresh result that got no word))
ROWS = [
    ("fresh", None, (1, 1), True),
    ("fresh", None, (2, 2), True),
    ("residual", None, (1, 1), True),
    ("residual", "match", (1, 1), True),           # not strided: the mark is not asked
    ("residual", "match", (2, 2), True),
    ("residual", None, (2, 2), False),
    ("residual", "stale", (2, 2), False),
    ("residual", (2, 1), (2, 2), False),
    ("residual", (3, 3), (2, 2), False),
    ("residual", "match", (2, 1), False),          # the same tensor scattered into with another geometry
    ("view", None, (1, 1), False),                 # identity, not equality of the bytes
    ("view", "match", (2, 2), False),
    ("other", None, (1, 1), False),
    ("other", "match", (2, 2), False),
    ("none", None, (1, 1), False),
    ("none", "match", (2, 2), False),
]
# (H3_TAGS, emit_amax, math name) -> does the column follow the table (else: never emits)
COLUMNS = [
    (True, None, "MATH_F16X3", True),
    (True, None, "MATH_F16", True),
    (True, True, "MATH_F16X3", True),
    (True, True, "MATH_F32", True),                # an fp32-kernel producer tags its output when asked to
    (True, None, "MATH_F32", False),
    (True, None, "MATH_BF16X6", False),
    (True, False, "MATH_F16X3", False),
    (True, False, "MATH_F16", False),
    (False, None, "MATH_F16X3", False),
    (False, True, "MATH_F16X3", False),
    (False, True, "MATH_F16", False),
]


@pytest.mark.parametrize("tags,emit_amax,math,follows", COLUMNS)
def test_output_word_truth_table(tags, emit_amax, math, follows, monkeypatch):
    from abr_iod_amd import ops
    monkeypatch.setattr(ops, "H3_TAGS", tags)
    for kind, mark, (sh, sw), emits in ROWS:
        out, residual = _case(kind, mark)
        got = ops.conv_out_emits(out, residual, sh, sw, emit_amax, getattr(ops, math))
        assert got is (emits and follows), (kind, mark, sh, sw, tags, emit_amax, math, got)


@pytest.mark.parametrize("emitted", [True, False])
def test_what_happens_to_the_result_after_the_launch(emitted):
    """a word written -> the result is tagged with it; none -> a caller's `out` loses its tag and its scatter mark, a fresh result is left
    alone; a fresh strided result is marked (data_ptr, sh, sw) either way, and a second pass that emitted keeps the mark it matched"""
    from abr_iod_amd import ops
    word, epoch = (0x1000, 7) if emitted else (None, 0)
    for kind, mark, (sh, sw), _ in ROWS:
        out, _r = _case(kind, mark)
        fresh = out is None
        if fresh:
            out = _t()
        else:
            ops.amax_tag(out, 0x2000, 3)           # whatever the caller's tensor carried before
        before = getattr(out, "_abr_scatter", None)
        assert ops.conv_out_done(out, fresh, word, epoch, sh, sw) is out
        assert ops.amax_of(out) == ((0x1000, 7) if emitted else (None, 0)), (kind, mark, sh, sw)
        if fresh:
            want = (out.data_ptr(), sh, sw) if (sh, sw) != (1, 1) else None
        else:
            want = before if emitted else None
        assert getattr(out, "_abr_scatter", None) == want, (kind, mark, sh, sw)
