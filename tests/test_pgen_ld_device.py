"""LD-compressed ``.pgen`` records on the GPU (``sai convert --out-pfile --ld-compress``): the kernels of
``sai_pgen_encode_ld`` against their host twin on every case of ``pgen_ld_cases`` (record types, lengths, status values
and record bytes identical, nothing written outside the batch's bytes), records at every residue, segments past the
grid cap, the written records through ``sai_pgen_decode`` and the pack2 decoder, ``convert`` on the GPU route against
the host route, and ``score`` on an LD-compressed fileset against ``score`` on the VCF it came from."""

import ctypes as C

import numpy as np
import pytest

import pgen_export_cases as PC
import pgen_ld_cases as LC
from test_pgen_export_cpu import fileset_bytes
from test_pgen_ld_cpu import base_rows, panel_config, panel_vcf, record_types_of

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes before and behind the records, elements behind every table, that must stay as they were


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


def encode_device(eng, block, ploidies, lead=0):
    """One ``sai_pgen_encode_ld`` call -> (records, vrtype, length, status), the records written from byte ``lead`` of a
    16-byte aligned address; what lies around the outputs is checked here."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer, pgen_writer

    lib = pgen_writer.load_ld()
    n_rows, n_slots = block.shape
    cap = n_rows * ((n_slots + 3) // 4)
    uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
    d_in = torch.from_numpy(np.ascontiguousarray(block)).to(eng.device)
    d_pl = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
    d_out = torch.full((GUARD + lead + cap + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_vt = torch.full((n_rows + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_len = torch.full((n_rows + GUARD,), -5, dtype=torch.int32, device=eng.device)
    d_off = torch.full((n_rows + 1 + GUARD,), -5, dtype=torch.int32, device=eng.device)
    d_st = torch.full((n_rows + GUARD,), -5, dtype=torch.int32, device=eng.device)
    assert d_out.data_ptr() % 16 == 0
    _ffi.check(lib.sai_pgen_encode_ld(eng.ctx, eng._ptr(d_in), n_rows, n_slots, eng._ptr(d_pl), uniform, C.c_void_p(d_out.data_ptr() + GUARD + lead),
                                      eng._ptr(d_vt), eng._ptr(d_len), eng._ptr(d_off), eng._ptr(d_st), pgen_writer.ENCODE_ALL,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    out, vt, ln, off, st = (t.cpu().numpy() for t in (d_out, d_vt, d_len, d_off, d_st))
    ln, off = ln.view(np.uint32), off.view(np.uint32)
    total = int(off[n_rows])
    assert (vt[n_rows:] == 0xA5).all() and (ln[n_rows:] == 0xFFFFFFFB).all() and (off[n_rows + 1 :] == 0xFFFFFFFB).all() and (st[n_rows:] == -5).all()
    assert total == int(ln[:n_rows].sum(dtype=np.uint64)) <= cap and off[:n_rows].tolist() == (np.cumsum(ln[:n_rows], dtype=np.uint64) - ln[:n_rows]).tolist()
    first = GUARD + lead
    assert (out[:first] == 0xA5).all() and (out[first + total :] == 0xA5).all()  # nothing before the records, nothing behind them
    return out[first : first + total], vt[:n_rows], ln[:n_rows], st[:n_rows]


_twin = {}


def twin(key, block, ploidies):
    """The host twin's answer, once per ``key``."""
    from sai_amd.utils import pgen_writer

    if key not in _twin:
        _twin[key] = pgen_writer.encode_host(block, ploidies, ld_compress=True)
    return _twin[key]


def same_as_host(eng, block, ploidies, name, lead=0):
    want = twin(name, block, ploidies)
    got = encode_device(eng, block, ploidies, lead)
    for label, a, b in zip(("vrtype", "length", "status", "records"), (got[1], got[2], got[3], got[0]), (want[1], want[2], want[3], want[0])):
        assert np.array_equal(a, b), (name, label)
    return want


@pytest.mark.parametrize("case", LC.CASES, ids=LC.CASE_IDS)
def test_kernels_equal_host_twin(eng, case):
    out, vrtype, length, status = same_as_host(eng, case.block, case.ploidies, case.name)
    assert not status.any()
    if "types" in case.want:  # the twin is pinned to the test writer on the host; once more here
        types, records, _ = LC.reference(case)
        assert vrtype.tolist() == types == case.want["types"] and out.tobytes() == b"".join(records)


def test_kernels_flag_what_the_host_twin_flags(eng):
    for name, block, ploidies, _, want_status in LC.unfit_cases():
        out, vrtype, length, status = same_as_host(eng, block, ploidies, name)
        assert status.tolist() == want_status and {2, 3} & set(vrtype.tolist()), name


def test_records_at_every_residue(eng):
    """The records of a call from every byte mod 4 of an aligned address, and within a call records of types 2 and 3
    that start at every residue."""
    case = next(c for c in LC.CASES if c.name == "33 rows x 83")
    for lead in range(4):
        out, vrtype, length, _ = same_as_host(eng, case.block, case.ploidies, case.name, lead)
    starts = np.cumsum(length) - length
    assert {int(s) % 4 for s, t in zip(starts, vrtype) if t in (2, 3)} == {0, 1, 2, 3}
    assert {int(s) % 4 for s, t in zip(starts, vrtype) if t not in (2, 3)} == {0, 1, 2, 3}


def test_segments_past_the_grid_cap(eng):
    """2 x cap + 3 segments of 5 samples: every workgroup of the plan kernel takes a third segment, the last one short."""
    from sai_amd.utils import pgen_writer

    cap = pgen_writer.load().sai_pgen_encode_grid_cap(eng.ctx)
    assert 0 < cap <= 1 << 16
    n_rows = (2 * cap + 3) * LC.SEGMENT - 9
    rng = np.random.default_rng(cap)
    codes = rng.integers(0, 3, (n_rows, 5)).astype(np.uint8)
    copies = rng.random(n_rows) < 0.5  # half of the rows repeat the row before
    copies[0] = False
    for r in np.flatnonzero(copies):
        codes[r] = codes[r - 1]
    out, vrtype, length, status = same_as_host(eng, PC.block_of(codes, 2), 2, "grid cap")
    assert not status.any() and not np.isin(vrtype[:: LC.SEGMENT], (2, 3)).any()
    for part in (vrtype[: cap * LC.SEGMENT], vrtype[2 * cap * LC.SEGMENT :]):
        assert 2 in part.tolist() and 0 in part.tolist()


ROUND_TRIP = [c for c in LC.SMALL if c.family in ("rows", "chain", "entries", "ploidies", "wide") or c.codes.shape[1] in (1, 5, 17, 257, 1025, 16385)]


def tables_of(vrtype, length):
    """rec and base [n][3] of records that stand back to back from byte 0."""
    ends = np.cumsum(length, dtype=np.int64)
    rec = np.ascontiguousarray(np.stack([ends - length, length.astype(np.int64), vrtype.astype(np.int64)], axis=1))
    base = np.full((len(vrtype), 3), -1, dtype=np.int64)
    for r, b in enumerate(base_rows(vrtype)):
        if b >= 0:
            base[r] = rec[b]
    return rec, base


@pytest.mark.parametrize("case", ROUND_TRIP, ids=[c.name for c in ROUND_TRIP])
def test_round_trip_through_the_device_decoders(eng, case):
    """``sai_pgen_decode`` gives the block back; ``sai_pgen_pack2`` gives its 2-bit form (one ploidy per call)."""
    import torch

    from sai_amd import _ffi, _ffi_pgen
    from test_bed_pack2_cpu import pack_numpy
    from test_pgen_pack2_device import DeviceCall

    lib = _ffi_pgen.load()
    out, vrtype, length, _ = twin(case.name, case.block, case.ploidies)  # the kernels' bytes: test_kernels_equal_host_twin
    n_rows, n = case.block.shape
    rec, base = tables_of(vrtype, length)
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    d_bytes, d_rec, d_base, d_flip = dev(np.ascontiguousarray(out)), dev(rec), dev(base), dev(np.zeros(n_rows, dtype=np.uint8))
    d_pl = dev(np.array(np.broadcast_to(np.asarray(case.ploidies, dtype=np.int32), (n,))))
    d_out = torch.empty((n_rows, n), dtype=torch.int8, device=eng.device)
    d_st = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_decode(eng.ctx, eng._ptr(d_bytes), out.size, n_rows, eng._ptr(d_rec), eng._ptr(d_base), eng._ptr(d_flip), n, n, None, 0,
                                   eng._ptr(d_pl), 0, C.c_void_p(d_out.data_ptr()), 0, eng._ptr(d_st), C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    assert not d_st.any() and np.array_equal(d_out.cpu().numpy(), case.block)
    if np.ndim(case.ploidies) == 0:
        call = DeviceCall(eng, out.tobytes(), rec, base, np.zeros(n_rows, dtype=np.uint8), n, np.arange(n, dtype=np.int32), 0, int(case.ploidies))
        packed = call.run(0, n_rows)
        assert not call.status.any() and not call.unfit.any()
        assert np.array_equal(packed, pack_numpy(np.where(case.block < 0, 3, case.block).astype(np.uint8)))


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import pgen_writer

    lib = pgen_writer.load_ld()
    assert lib.sai_pgen_export_ld_version() == 1 and lib.sai_pgen_ld_segment() == LC.SEGMENT and lib.sai_pgen_export_abi_version() == 1
    d_in = torch.zeros((64,), dtype=torch.int8, device=eng.device)
    d_out = torch.full((64,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_vt = torch.full((8,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_len, d_off, d_st = (torch.full((8,), -5, dtype=torch.int32, device=eng.device) for _ in range(3))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = (eng.ctx, ptr(d_in), 2, 5, None, 2, ptr(d_out), ptr(d_vt), ptr(d_len), ptr(d_off), ptr(d_st), pgen_writer.ENCODE_ALL)
    refused = [
        ({0: None}, b"ctx is NULL"), ({1: None}, b"NULL buffer"), ({6: None}, b"NULL buffer"), ({7: None}, b"NULL buffer"), ({8: None}, b"NULL buffer"),
        ({9: None}, b"NULL buffer"), ({10: None}, b"NULL buffer"), ({5: 0}, b"NULL buffer"),
        ({2: -1}, b"size out of range"), ({3: 0}, b"size out of range: a .pgen record holds 1 to 2^31 - 1 samples"),
        ({5: 3}, b"uniform_ploidy must be 0, 1 or 2"), ({11: 0}, b"stages must be 1 .. 7"), ({11: 8}, b"stages must be 1 .. 7"), ({1: ptr(d_in, 1)}, b"dosage must be 16-byte aligned"),
        ({2: (1 << 32) // 501 + 1, 3: 2002}, b"a call writes less than 4 GiB of records"),
    ]  # fmt: skip
    for change, message in refused:
        args = [change.get(k, v) for k, v in enumerate(good)]
        assert lib.sai_pgen_encode_ld(*args, stream) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), (change, message)
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all() and (d_vt == 0xA5).all() and (d_len == -5).all() and (d_off == -5).all() and (d_st == -5).all()
    assert lib.sai_pgen_encode_ld(eng.ctx, None, 0, 5, None, 2, None, None, None, ptr(d_off), None, 7, stream) == 0  # no row: the total is 0
    torch.cuda.synchronize()
    assert d_off.tolist() == [0] + [-5] * 7 and (d_out == 0xA5).all()
    _ffi.check(lib.sai_pgen_encode_ld(*good, stream))  # two rows of zeros: a type 4 anchor without an entry, a type 2 row without one
    torch.cuda.synchronize()
    assert d_vt.tolist()[:3] == [4, 2, 0xA5] and d_off.tolist()[:4] == [0, 1, 2, -5] and d_out[:3].tolist() == [0, 0, 0xA5] and d_st.tolist()[:3] == [0, 0, -5]


# ---- convert and score on the GPU route ----


def convert_both(monkeypatch, tmp_path, vcf, chrom, tag="", **kw):
    """The LD-compressed fileset written on the GPU route and on the host route -> (prefix, prefix, summary)."""
    from sai_amd.sai import convert

    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    host = convert(vcf, chrom, out_pfile=str(tmp_path / f"host{tag}"), ld_compress=True, **kw)
    monkeypatch.delenv("SAI_AMD_INGEST")
    device = convert(vcf, chrom, out_pfile=str(tmp_path / f"device{tag}"), ld_compress=True, **kw)
    assert {k: v for k, v in host.items() if k != "ms"} == {k: v for k, v in device.items() if k != "ms"}
    assert device["ms"]["encode"] > 0 and device["ms"]["d2h"] > 0 and host["ms"]["d2h"] == 0
    return str(tmp_path / f"device{tag}"), str(tmp_path / f"host{tag}"), device


def test_convert_on_the_gpu_writes_the_files_of_the_host_route(eng, in_repo_root, tmp_path, monkeypatch):
    vcf, codes = panel_vcf(tmp_path)
    device, host, summary = convert_both(monkeypatch, tmp_path, vcf, "9")
    assert fileset_bytes(device) == fileset_bytes(host)
    assert open(device + ".pgen", "rb").read() == LC.reference_of("panel vcf", codes)[2]
    assert summary["record_types"] == record_types_of(device, len(codes)) and summary["record_types"][2] > 0 and summary["record_types"][3] > 0
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")  # 16 rows per batch: both pinned buffers go round many times
    small, _, _ = convert_both(monkeypatch, tmp_path, vcf, "9", tag="_small")
    assert fileset_bytes(small) == fileset_bytes(host)


def score_files(source, cfgfile, out, layout):
    from sai_amd.sai import score

    score(vcf_file=source, chr_name="9", win_len=20000, win_step=10000, anc_allele_file=None, output_file=str(out), config=cfgfile, num_workers=1,
          layout=layout)  # fmt: skip
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


@pytest.mark.parametrize("layout", ["int8", "packed2"])
def test_score_on_the_ld_compressed_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, layout):
    """TSV and logs byte for byte; the fileset holds records of type 2 and of type 3."""
    from sai_amd.sai import convert

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    vcf, codes = panel_vcf(tmp_path)
    cfgfile = panel_config(tmp_path, codes.shape[1])
    prefix = str(tmp_path / "ld")
    summary = convert(vcf, "9", out_pfile=prefix, ld_compress=True)
    assert summary["record_types"][2] > 0 and summary["record_types"][3] > 0 and record_types_of(prefix, len(codes)) == summary["record_types"]
    want = score_files(vcf, cfgfile, tmp_path / "vcf" / "s.tsv", None)
    assert score_files(prefix + ".pgen", cfgfile, tmp_path / "set" / "s.tsv", layout) == want and len(want[".tsv"].splitlines()) > 1
