"""sai_tokenize_gt itself, called as sai_amd/utils/_ingest.py calls it, on the hand-built buffers of
tests/tokenize_cases.py: fields that start at every (step, lane, byte) of three steps and more, lines that end on and
around a step boundary, a line of 5 000 columns, fields across a step boundary, the genotype rules one line each,
launches of 1 .. 9 lines that end 0 .. 3 bytes before the end of the buffer.  Status and row bytes are compared exactly
with the statement of the rules that test_tokenize_cases_cpu.py pins to the host reader; rows and status entries
behind the last line must stay as they were."""

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import tokenize_cases as tc

pytestmark = pytest.mark.gpu

GUARD_ROWS = 2  # rows and status entries behind the last line, which no launch may touch


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


def device_arguments(eng, case):
    """The device tensors of a case, ``out`` prefilled with the sentinel and ``status`` with -1, GUARD_ROWS longer than
    the launch."""
    import torch

    tc.check_contract(case)  # a table that points outside the buffer is a bug of the test, and faults the GPU
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    t = SimpleNamespace()
    t.text = up(np.frombuffer(case.text, dtype=np.uint8).copy())
    t.off, t.len, t.flip, t.gi = up(case.off), up(case.len), up(case.flip), up(case.gi)
    t.slots, t.ploidy = up(case.slot_of_col), up(case.ploidy)
    t.out = torch.full((case.n_lines + GUARD_ROWS, case.n_out), tc.SENTINEL, dtype=torch.int8, device=eng.device)
    t.status = torch.full((case.n_lines + GUARD_ROWS,), -1, dtype=torch.int32, device=eng.device)
    assert t.text.data_ptr() % 4 == 0 and t.text.numel() % 4 == 0
    return t


def call(eng, case, t, **replace):
    """One call of the entry point with the arguments of ``case``; ``replace`` swaps single arguments."""
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    a = dict(text=ptr(t.text), n_text=t.text.numel(), n_lines=case.n_lines, off=ptr(t.off), len=ptr(t.len), flip=ptr(t.flip), gi=ptr(t.gi),
             n_cols=case.n_cols, slots=ptr(t.slots), n_out=case.n_out, ploidy=ptr(t.ploidy), out=ptr(t.out), status=ptr(t.status))  # fmt: skip
    a.update(replace)
    return eng.lib.sai_tokenize_gt(eng.ctx, a["text"], a["n_text"], a["n_lines"], a["off"], a["len"], a["flip"], a["gi"], a["n_cols"],
                                   a["slots"], a["n_out"], a["ploidy"], a["out"], a["status"], None)  # fmt: skip


def run_case(eng, case):
    """Launch a case once and compare everything the launch may and may not write."""
    import torch

    t = device_arguments(eng, case)
    assert call(eng, case, t) == 0, eng.lib.sai_last_error().decode()
    torch.cuda.synchronize()
    status, out, n = t.status.cpu().numpy(), t.out.cpu().numpy(), case.n_lines
    wrong = np.flatnonzero(status[:n] != case.status)
    assert len(wrong) == 0, (case.name, "status", len(wrong), int(wrong[0]), int(status[wrong[0]]), case.why[wrong[0]], vars(case.lines[wrong[0]]))
    assert (status[n:] == -1).all(), (case.name, "status behind the last line")
    kept = case.status == 0
    wrong = np.flatnonzero(kept & (out[:n] != case.rows).any(axis=1))
    if len(wrong):
        i = int(wrong[0])
        slots = np.flatnonzero(out[i] != case.rows[i])
        cols = [int(np.flatnonzero(case.slot_of_col == s)[0]) if (case.slot_of_col == s).any() else None for s in slots[:6]]
        raise AssertionError((case.name, "rows", len(wrong), i, vars(case.lines[i]), "slots", slots[:6].tolist(), "columns", cols,
                              "got", out[i][slots[:6]].tolist(), "want", case.rows[i][slots[:6]].tolist()))  # fmt: skip
    assert (out[n:] == tc.SENTINEL).all(), (case.name, "rows behind the last line")


def test_fields_start_at_every_lane_and_byte_of_three_steps(eng):
    """The whole sweep in one launch: 6 216 lines, every column selected."""
    run_case(eng, tc.sweep_case())


@pytest.mark.parametrize("name", ["line_ends", "straddle", "long_all_columns", "long_every_97th"])
def test_line_geometry(eng, name):
    run_case(eng, next(c for c in tc.all_cases() if c.name == name))


def test_rules_one_line_each(eng):
    tables = tc.rules_cases()
    assert [c.name for c in tables] == ["rules", "rules_ploidy_63_64", "rules_ploidy_128_129", "empty_1col", "empty_2col"]
    for case in tables:
        assert case.status.any() or case.name == "empty_1col"
        run_case(eng, case)


def test_launch_shapes(eng):
    """1, 3, 4, 5 and 9 lines back to back (four lines per workgroup), the last one ending 0 .. 3 bytes before the end of
    the buffer: one launch each."""
    cases = tc.launch_cases()
    assert len(cases) == 20
    for case in cases:
        run_case(eng, case)


def test_argument_errors_and_the_empty_launch(eng):
    import torch

    from sai_amd import _ffi

    case = tc.launch_cases()[0]
    t = device_arguments(eng, case)

    def refused(message, **replace):
        assert call(eng, case, t, **replace) == _ffi.SAI_ERR_ARG, replace
        assert message in eng.lib.sai_last_error().decode(), (replace, eng.lib.sai_last_error().decode())

    refused("4-byte aligned", text=C.c_void_p(t.text.data_ptr() + 1), n_text=t.text.numel() - 4)
    for n_text in (t.text.numel() - 1, t.text.numel() - 2, t.text.numel() - 3):
        refused("multiple of 4", n_text=n_text)
    for n_out in (0, -1):
        refused("size out of range", n_out=n_out)
    refused("size out of range", n_lines=-1)
    refused("size out of range", n_cols=-1)
    refused("size out of range", n_text=-4)
    for name in ("text", "off", "len", "flip", "gi", "slots", "ploidy", "out", "status"):
        refused("NULL buffer", **{name: None})
    # no line: SAI_OK before anything is looked at, whatever the other arguments hold
    assert call(eng, case, t, n_lines=0) == 0
    assert call(eng, case, t, n_lines=0, text=None, off=None, out=None, status=None, n_text=3) == 0
    torch.cuda.synchronize()
    assert (t.out.cpu().numpy() == tc.SENTINEL).all() and (t.status.cpu().numpy() == -1).all()  # nothing ran in all of the above
    assert call(eng, case, t) == 0  # and the same arguments, unchanged, are a good launch
    torch.cuda.synchronize()
    assert t.status.cpu().numpy().tolist() == case.status.tolist() + [-1] * GUARD_ROWS
    assert np.array_equal(t.out.cpu().numpy()[: case.n_lines], case.rows)
