"""sai_text_line_starts / sai_text_line_heads on batches of 4 to 12 MB (tests/scan_cases.py): the one-workgroup scan of
the 4 KiB blocks' newline counts gives every thread two or three blocks there, and threads whose range starts beyond
the last block occur -- test_line_table_kernels stops where every thread has one block.  Exact comparisons with the
numpy statement; canaries behind every output."""

import ctypes as C

import numpy as np
import pytest

import scan_cases as sc

pytestmark = pytest.mark.gpu

FILL = -7


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


def p(t, o=0):
    return C.c_void_p(t.data_ptr() + o)


def line_starts(eng, case, capacity):
    """(info, starts, line words, scratch) after sai_text_line_starts; the text lies at the case's misalignment with
    newlines in front of it and behind it that must not count."""
    import torch

    from sai_amd import _ffi

    n, mis = len(case.text), case.mis
    d_text = torch.full((mis + n + 48,), 10, dtype=torch.uint8, device=eng.device)
    d_text[mis : mis + n] = torch.from_numpy(np.frombuffer(case.text, dtype=np.uint8).copy()).to(eng.device)
    assert d_text.data_ptr() % 16 == 0
    d_starts = torch.full((capacity + 1 + 8,), FILL, dtype=torch.int64, device=eng.device)
    d_words = torch.full((capacity + 8,), FILL, dtype=torch.int32, device=eng.device)
    d_scr = torch.full((case.n_blocks + 1 + 8,), FILL, dtype=torch.int32, device=eng.device)
    d_info = torch.full((3 + 5,), FILL, dtype=torch.int32, device=eng.device)
    _ffi.check(eng.lib.sai_text_line_starts(eng.ctx, p(d_text, mis), n, capacity, p(d_starts), p(d_words), p(d_scr), p(d_info), None))
    torch.cuda.synchronize()
    return d_text, d_info.cpu().numpy(), d_starts, d_words.cpu().numpy(), d_scr.cpu().numpy()


def check_scratch(case, scr):
    """The scan's own output: the exclusive running sum of the blocks' newline counts, the total behind it."""
    per_block = np.bincount((case.starts[1:] - 1 + case.mis) // sc.LINE_BLOCK, minlength=case.n_blocks)
    want = np.concatenate([[0], np.cumsum(per_block)])
    assert scr[: case.n_blocks + 1].tolist() == want.tolist()
    assert (scr[case.n_blocks + 1 :] == FILL).all()


@pytest.mark.parametrize("mis", sc.LINE_MIS)
@pytest.mark.parametrize("n_blocks", sc.LINE_BLOCKS)
def test_line_table_of_a_large_batch(eng, n_blocks, mis):
    import torch

    from sai_amd import _ffi

    case = sc.line_case(n_blocks, mis)
    n_l = case.n_lines
    cap = n_l + 5
    d_text, info, d_starts, words, scr = line_starts(eng, case, cap)
    assert info[:3].tolist() == [n_l, int((case.words & 0x7FFFFFFF).max()), 0] and (info[3:] == FILL).all()
    check_scratch(case, scr)
    starts = d_starts.cpu().numpy()
    assert np.array_equal(starts[: n_l + 1], case.starts)
    assert (starts[n_l + 1 :] == FILL).all()
    assert np.array_equal(words[:n_l].astype(np.int64) & 0xFFFFFFFF, case.words)
    assert (words[n_l:] == FILL).all()
    hb = sc.HEAD_BYTES
    d_heads = torch.full((n_l * hb + 16,), 0x55, dtype=torch.uint8, device=eng.device)
    _ffi.check(eng.lib.sai_text_line_heads(eng.ctx, p(d_text, mis), len(case.text), p(d_starts), n_l, hb, p(d_heads), None))
    heads = d_heads.cpu().numpy()
    assert np.array_equal(heads[: n_l * hb].reshape(n_l, hb), case.heads(hb))
    assert (heads[n_l * hb :] == 0x55).all()


def test_line_capacity_too_small_in_a_large_batch(eng):
    """More than 1 024 blocks and room for half the lines: the flag is set, the count is that of all lines, and
    nothing is written beyond capacity + 1 starts and capacity line words."""
    case = sc.line_case(1025, 7)
    cap = case.n_lines // 2
    _, info, d_starts, words, scr = line_starts(eng, case, cap)
    assert info[:3].tolist() == [case.n_lines, int((case.words[:cap] & 0x7FFFFFFF).max()), 1] and (info[3:] == FILL).all()
    check_scratch(case, scr)
    starts = d_starts.cpu().numpy()
    assert np.array_equal(starts[: cap + 1], case.starts[: cap + 1])
    assert (starts[cap + 1 :] == FILL).all()
    assert np.array_equal(words[:cap].astype(np.int64) & 0xFFFFFFFF, case.words[:cap])
    assert (words[cap:] == FILL).all()
