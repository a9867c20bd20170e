"""The .csi index of a BCF file on the GPU: ``load_dosage_device`` through the GPU route with the index against the same
route without it and against the host route, for the files and regions of tests/test_bcf_index_cpu.py; wrong indexes;
and ``score`` in four chunks with and without the index."""

import os

import numpy as np
import pytest

import csi_builder as X
import csi_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for name in ("SAI_AMD_BCF_INDEX", "SAI_AMD_GPU_INFLATE", "SAI_AMD_INGEST", "SAI_AMD_INFLATE_BATCH"):
        monkeypatch.delenv(name, raising=False)


def equal_reads(a, b) -> bool:
    block = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x)  # noqa: E731
    return a[0].tolist() == b[0].tolist() and block(a[1]).dtype == block(b[1]).dtype and np.array_equal(block(a[1]), block(b[1])) and tuple(a[2:]) == tuple(b[2:])


@pytest.mark.parametrize("batch", [None, 1400], ids=["one batch", "batches of two members"])
@pytest.mark.parametrize("min_shift,depth", K.LAYOUTS[:2])
def test_the_gpu_route_with_and_without_the_index(eng, tmp_path, monkeypatch, min_shift, depth, batch):
    """Blocks, positions, flips and counts.  The files are small, so by default the first batch is the whole tail;
    with batches of 1 400 inflated bytes a seeked read takes three or more of them and carries records over."""
    from sai_amd.utils import bcf

    path, plain = K.write_bcf(tmp_path / "a.bcf"), K.write_bcf(tmp_path / "plain.bcf")
    X.write_csi(path, min_shift, depth)
    recs, anc = K.records(path), K.anc_file(tmp_path / "anc.bed", path)
    order, ploidies = list(reversed(K.SAMPLES))[:4], [2, 1, 3, 2]
    if batch:
        monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", str(batch))
    made = flipped = 0
    for chrom, tid, step in (("2", 1, 3), ("1", 0, 11), ("3", 2, 11)):
        for k, (start, end) in enumerate(K.regions(recs, tid, min_shift, depth)[::step] + ([K.last_quarter(path)[0]] if tid == 1 else [])):
            a = anc if tid == 1 and k % 2 else None
            trace, without = {}, {}
            got = bcf.load_dosage_device(eng, path, chrom, order, ploidies, start, end, a, trace=trace)
            assert trace["route"] == "device", (chrom, start, end)
            unindexed = bcf.load_dosage_device(eng, plain, chrom, order, ploidies, start, end, a, trace=without)
            assert without["route"] == "device" and not without["seek"]["made"]
            want = bcf.load_dosage(plain, chrom, order, ploidies, start, end, a)
            assert equal_reads(got, want) and equal_reads(unindexed, want), (chrom, start, end, a)
            made += trace["seek"]["made"]
            flipped += a is not None and len(want[0]) > 0
            if trace["seek"]["made"]:
                assert trace["seek"]["file_bytes"] <= without["seek"]["file_bytes"]
    assert made > 30 and flipped > 5
    # the last-quarter region: the offset, fewer bytes of the file, and three or more batches with a carry where they are small
    (start, end), first = K.last_quarter(path)
    trace, without = {"serial": True}, {}
    got = bcf.load_dosage_device(eng, path, "2", order, ploidies, start, end, trace=trace)
    bcf.load_dosage_device(eng, plain, "2", order, ploidies, start, end, trace=without)
    size = os.path.getsize(path)
    print("file", size, "bytes;", trace["seek"], "without the index", without["seek"])
    if start - 1 >= 1 << (min_shift + 3 * depth):  # beyond the range of this index: walked from the start, as without one
        assert trace["route"] == "device" and not trace["seek"]["made"] and (min_shift, depth) == (6, 2)
        bcf.release_buffers(eng)
        return
    assert trace["route"] == "device" and trace["seek"]["made"] and 0 < trace["seek"]["voffset"] <= first["voff"]
    # without the index the read gets at least as far as the region's first record, which lies behind 3/4 of the file
    assert trace["seek"]["file_bytes"] < size / 2 and without["seek"]["file_bytes"] > 0.75 * size
    if batch:
        tail = sum(r["g_end"] - r["g"] for r in recs if r["voff"] >= trace["seek"]["voffset"] and r["chrom"] == 1)
        assert tail >= 3 * batch  # three or more batches; a record of ~55 bytes never ends on every multiple of 1 400: a carry
    # the knob
    monkeypatch.setenv("SAI_AMD_BCF_INDEX", "0")
    trace = {}
    assert equal_reads(bcf.load_dosage_device(eng, path, "2", order, ploidies, start, end, trace=trace), got) and not trace["seek"]["made"]
    monkeypatch.setenv("SAI_AMD_BCF_INDEX", "1")
    # the host route of load_dosage_device takes the index too
    monkeypatch.setenv("SAI_AMD_GPU_INFLATE", "0")
    trace = {}
    assert equal_reads(bcf.load_dosage_device(eng, path, "2", order, ploidies, start, end, trace=trace), got)
    assert trace["route"] == "host" and trace["seek"]["made"] and trace["seek"]["file_bytes"] < size / 2
    bcf.release_buffers(eng)


def test_a_wrong_index_of_each_kind_still_gives_the_right_block(eng, tmp_path, monkeypatch):
    from sai_amd.utils import bcf

    path, other = K.write_bcf(tmp_path / "a.bcf", level=0), K.write_bcf(tmp_path / "b.bcf", level=0, rotate_ids=1)
    (start, end), _ = K.last_quarter(path)
    anc = K.anc_file(tmp_path / "anc.bed", path)
    ask = (eng, path, "2", K.SAMPLES, [2] * 5, start, end, anc)
    want = bcf.load_dosage(path, *ask[2:])
    assert len(want[0]) > 5
    X.write_csi(path, 4, 3)
    trace = {}
    assert equal_reads(bcf.load_dosage_device(*ask, trace=trace), want) and trace["seek"]["made"] and trace["route"] == "device"  # the control
    for name, write in K.wrong_indexes(path, other):
        write()
        for batch in (None, 1400):
            if batch:
                monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", str(batch))
            else:
                monkeypatch.delenv("SAI_AMD_INFLATE_BATCH", raising=False)
            trace = {}
            got = bcf.load_dosage_device(*ask, trace=trace)
            assert equal_reads(got, want), name
            assert trace["route"] == "device" and not trace["seek"]["made"], (name, trace["seek"])
    bcf.release_buffers(eng)


def test_score_in_four_chunks_is_the_same_with_and_without_the_index(eng, in_repo_root, tmp_path, monkeypatch):
    from test_bcf_device import score_files, seeded_block

    from sai_amd import sai as sai_mod
    from sai_amd.utils import bcf

    _, path, cfg, n_genotypes = seeded_block(tmp_path)
    win = (5000, 2500)
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES", raising=False)
    one = score_files(path, "4", cfg, None, tmp_path / "one" / "s.tsv", win)
    assert set(one) == {".tsv", ".U.log", ".Q.log"} and len(one[".tsv"].splitlines()) > 30
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(-(-n_genotypes // 4)))
    assert sai_mod.chunks_for_memory(path) == 4
    seeks = []
    real = bcf._load_device_walk

    def watched(*a, **k):
        trace = a[9] if len(a) > 9 and a[9] is not None else {}
        got = real(*a[:9], trace, *a[10:], **k)
        seeks.append(trace["seek"]["made"])
        return got

    monkeypatch.setattr(bcf, "_load_device_walk", watched)
    assert score_files(path, "4", cfg, None, tmp_path / "four" / "s.tsv", win) == one
    assert seeks and not any(seeks)
    del seeks[:]
    X.write_csi(path)
    assert score_files(path, "4", cfg, None, tmp_path / "four_indexed" / "s.tsv", win) == one
    assert sum(seeks) >= 3, seeks  # every chunk but the first begins at an offset of the index
    bcf.release_buffers(eng)
