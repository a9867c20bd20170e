"""A VCF's calls written as an EIGENSOFT fileset, on the GPU: the kernels ``sai_geno_encode`` and
``sai_geno_encode_transposed`` against their host twin byte for byte, ``convert`` on the GPU route against the host
route, and ``score`` on the converted fileset against ``score`` on the VCF (byte-identical files).

Neither grid is capped -- a lane of the packed kernel takes one 32-bit word of the records, a workgroup of the transposed
one a tile of 256 rows x 64 slots, and a call of 4 GiB is refused -- so there is no grid-stride loop to run past; the
refusal is tested instead.  The input of every call starts at a 16-byte boundary (an allocation of its own) while its
rows do not: 2 002 and 193 slots, among others, are no multiple of 16."""

import ctypes as C

import numpy as np
import pytest

import geno_export_cases as GC
from test_bed_export_cpu import mixed_case
from test_bed_export_device import SCORE_CASES, score_files
from test_geno_export_cpu import FORMATS, fileset_bytes

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes behind the records that must stay as they were


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


class Device:
    """A block on the device with its ploidies, and the two kernels on it; the bytes around ``out`` and the words
    behind ``status`` are checked after every call."""

    def __init__(self, eng, block, ploidies):
        import torch

        from sai_amd.utils import bed_writer, geno_writer

        self.eng, self.lib, self.torch = eng, geno_writer.load(), torch
        self.n_rows, self.n_slots = block.shape
        self.uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
        self.d_in = torch.from_numpy(np.ascontiguousarray(block)).to(eng.device)
        self.d_pl = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
        assert self.d_in.data_ptr() % 16 == 0
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _buffers(self, nbytes, status):
        # out sits 16 * k bytes into its allocation: a guard before it and one behind it
        d_out = self.torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=self.torch.uint8, device=self.eng.device)
        fill = np.concatenate([np.full(self.n_rows, -5, dtype=np.int32) if status is None else status, np.full(2, -5, dtype=np.int32)])
        return d_out, self.torch.from_numpy(fill).to(self.eng.device)

    def _collect(self, d_out, d_st, nbytes):
        self.torch.cuda.synchronize()
        out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        assert (out[:GUARD] == 0xA5).all() and (out[GUARD + nbytes :] == 0xA5).all() and (st[self.n_rows :] == -5).all()
        return out[GUARD : GUARD + nbytes], st[: self.n_rows]

    def packed(self):
        from sai_amd import _ffi

        rlen = GC.record_bytes(self.n_slots)
        d_out, d_st = self._buffers(self.n_rows * rlen, None)  # the entry point zeroes the status
        _ffi.check(self.lib.sai_geno_encode(self.eng.ctx, self.eng._ptr(self.d_in), self.n_rows, self.n_slots, self.eng._ptr(self.d_pl), self.uniform,
                                            C.c_void_p(d_out.data_ptr() + GUARD), self.eng._ptr(d_st), self.stream))  # fmt: skip
        out, st = self._collect(d_out, d_st, self.n_rows * rlen)
        return out.reshape(self.n_rows, rlen), st

    def transposed(self, slot0, n_out, status=None):
        """``status`` = the words as the calls before left them (default: zeros, as the converter starts them)."""
        from sai_amd import _ffi

        rlen = GC.record_bytes(self.n_rows)
        d_out, d_st = self._buffers(n_out * rlen, np.zeros(self.n_rows, dtype=np.int32) if status is None else status)
        _ffi.check(self.lib.sai_geno_encode_transposed(self.eng.ctx, self.eng._ptr(self.d_in), self.n_rows, self.n_slots, self.eng._ptr(self.d_pl), self.uniform,
                                                       slot0, n_out, C.c_void_p(d_out.data_ptr() + GUARD), self.eng._ptr(d_st), self.stream))  # fmt: skip
        out, st = self._collect(d_out, d_st, n_out * rlen)
        return out.reshape(n_out, rlen), st


@pytest.mark.parametrize("shape", GC.shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_the_host_twin(eng, shape):
    from sai_amd.utils.geno_writer import encode_host

    n_rows, n_slots = shape
    rng = np.random.default_rng(4000 * n_rows + n_slots)
    for name, ploidies in GC.ploidy_cases(rng, n_slots):
        for flagged in (False, True):
            block = GC.random_block(rng, n_rows, n_slots, ploidies)
            if flagged:
                GC.plant_unfit(rng, block, ploidies)
            dev = Device(eng, block, ploidies)
            want, want_status = encode_host(block, ploidies)
            records, status = dev.packed()
            assert np.array_equal(records, want) and status.tolist() == want_status.tolist() and bool(status.any()) == flagged, (name, flagged)
            want_t = encode_host(block, ploidies, transposed=True)[0]
            combined = np.zeros(n_rows, dtype=np.int32)
            for slot0, n_out in GC.slot_groups(n_slots):
                records, status = dev.transposed(slot0, n_out)
                want_part = encode_host(block, ploidies, transposed=True, slot0=slot0, n_out=n_out)[1]
                assert np.array_equal(records, want_t[slot0 : slot0 + n_out]) and status.tolist() == want_part.tolist(), (name, flagged, slot0, n_out)
            # the status of several calls, each raising what the one before left: the twin's over the whole block
            half = n_slots // 2
            for slot0, n_out in ((half, n_slots - half), (0, half)):
                if n_out:
                    combined = dev.transposed(slot0, n_out, status=combined)[1].copy()
            assert combined.tolist() == want_status.tolist()
            if shape in ((17, 13), (257, 65)):  # the twin is pinned to the numpy statement on the host; once more here
                assert np.array_equal(dev.packed()[0], GC.numpy_encode(block, ploidies)[0])
                assert np.array_equal(dev.transposed(0, n_slots)[0], GC.numpy_encode(block, ploidies, transposed=True)[0])


def test_every_byte_value_at_every_lane_position(eng):
    """All 256 values of a byte at both ploidies, at each of the 16 positions of a lane's load (packed) and at each of
    the four slots and four rows of a lane (transposed)."""
    from sai_amd.utils.geno_writer import encode_host

    values = np.arange(256, dtype=np.uint8).view(np.int8)
    for ploidy in (2, 1):
        block = np.zeros((256 * 16, 32), dtype=np.int8)
        for k in range(16):
            block[k * 256 : (k + 1) * 256, k] = values
            block[k * 256 : (k + 1) * 256, 16 + (k * 7) % 16] = values[::-1]
        dev = Device(eng, block, ploidy)
        for transposed in (False, True):
            want, want_status = encode_host(block, ploidy, transposed=transposed)
            records, status = dev.transposed(0, 32) if transposed else dev.packed()
            assert np.array_equal(records, want) and status.tolist() == want_status.tolist()
            assert np.array_equal(records, GC.numpy_encode(block, ploidy, transposed)[0])


def test_a_ploidy_outside_its_range(eng):
    from sai_amd.utils.geno_writer import encode_host

    rng = np.random.default_rng(33)
    for n_slots in (33, 201):
        ploidies = rng.integers(1, 3, n_slots).astype(np.int32)
        for where in (0, n_slots // 2, n_slots - 1):
            pl = ploidies.copy()
            pl[where] = 7
            block = GC.plant_unfit(rng, GC.random_block(rng, 9, n_slots, ploidies), ploidies)
            dev = Device(eng, block, pl)
            for transposed in (False, True):
                want, want_status = encode_host(block, pl, transposed=transposed)
                records, status = dev.transposed(0, n_slots) if transposed else dev.packed()
                assert np.array_equal(records, want) and status.tolist() == want_status.tolist() == [GC.BAD_INDEX] * 9
            # a slot group without the bad ploidy does not say so
            if where == 0:
                want_part = encode_host(block, pl, transposed=True, slot0=1, n_out=n_slots - 1)[1]
                assert dev.transposed(1, n_slots - 1)[1].tolist() == want_part.tolist() and GC.BAD_INDEX not in want_part.tolist()


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import geno_writer

    lib = geno_writer.load()
    d_in = torch.zeros((64,), dtype=torch.int8, device=eng.device)
    d_out = torch.full((512,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_st = torch.full((4,), -5, dtype=torch.int32, device=eng.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = (eng.ctx, ptr(d_in), 2, 5, None, 2, ptr(d_out), ptr(d_st))
    refused = [
        ({0: None}, b"ctx is NULL"), ({1: None}, b"NULL buffer"), ({6: None}, b"NULL buffer"), ({7: None}, b"NULL buffer"), ({5: 0}, b"NULL buffer"),
        ({2: -1}, b"size out of range"), ({3: 0}, b"size out of range"), ({5: 3}, b"uniform_ploidy must be 0, 1 or 2"),
        ({1: ptr(d_in, 1)}, b"dosage must be 16-byte aligned"), ({6: ptr(d_out, 4)}, b"out must be 16-byte aligned"),
        ({2: (1 << 32) // 501 + 1, 3: 2002}, b"a call writes less than 4 GiB of records"),
    ]  # fmt: skip
    for change, message in refused:
        args = [change.get(k, v) for k, v in enumerate(good)]
        assert lib.sai_geno_encode(*args, stream) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), message
    good_t = (eng.ctx, ptr(d_in), 2, 5, None, 2, 0, 5, ptr(d_out), ptr(d_st))
    refused_t = [
        ({0: None}, b"ctx is NULL"), ({1: None}, b"NULL buffer"), ({8: None}, b"NULL buffer"), ({9: None}, b"NULL buffer"), ({5: 0}, b"NULL buffer"),
        ({2: -1}, b"size out of range"), ({3: 0}, b"size out of range"), ({5: 3}, b"uniform_ploidy must be 0, 1 or 2"),
        ({6: 1}, b"slot0 + n_out exceeds n_slots"), ({6: -1}, b"slot0 + n_out exceeds n_slots"), ({7: 6}, b"slot0 + n_out exceeds n_slots"),
        ({1: ptr(d_in, 1)}, b"dosage must be 16-byte aligned"), ({8: ptr(d_out, 4)}, b"out must be 16-byte aligned"),
        ({2: 1 << 33, 3: 70000, 7: 3}, b"a call writes less than 4 GiB of records"),
    ]  # fmt: skip
    for change, message in refused_t:
        args = [change.get(k, v) for k, v in enumerate(good_t)]
        assert lib.sai_geno_encode_transposed(*args, stream) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), message
    assert lib.sai_geno_encode(eng.ctx, None, 0, 5, None, 2, None, None, stream) == 0  # no row: fine, nothing touched
    assert lib.sai_geno_encode_transposed(eng.ctx, ptr(d_in), 2, 5, None, 2, 3, 0, None, None, stream) == 0  # no slot: the same
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all() and (d_st == -5).all()


# ---- convert on the GPU route ----


def convert_both(monkeypatch, tmp_path, vcf, chrom, **kw):
    """The fileset written on the GPU route and on the host route -> (prefix, prefix)."""
    from sai_amd.sai import convert

    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    host = convert(vcf, chrom, out_eigenstrat=str(tmp_path / "host"), **kw)
    monkeypatch.delenv("SAI_AMD_INGEST")
    device = convert(vcf, chrom, out_eigenstrat=str(tmp_path / "device"), **kw)
    assert {k: v for k, v in host.items() if k != "ms"} == {k: v for k, v in device.items() if k != "ms"}
    assert device["ms"]["encode"] > 0 and device["ms"]["d2h"] > 0 and host["ms"]["d2h"] == 0
    return str(tmp_path / "device"), str(tmp_path / "host")


@pytest.mark.parametrize("batch", [None, 200])
@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_on_the_gpu_writes_the_files_of_the_host_route(eng, in_repo_root, tmp_path, monkeypatch, fmt, batch):
    """13 samples and 100 rows, records of 48 bytes.  A budget of 200 bytes is 16 rows of the packed form a batch (the
    least) -- 7 batches, the last of 4 rows -- and 4 individuals of the transposed one -- 4 batches, the last of 1:
    both pinned buffers go round more than once.  Then a call that does not fit: the words of the host route."""
    from sai_amd.sai import convert

    case = mixed_case(tmp_path)
    if batch is not None:
        monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", str(batch))
    device, host = convert_both(monkeypatch, tmp_path, case["vcf"], "7", geno_format=fmt, haploid_samples=case["haploid"])
    assert fileset_bytes(device) == fileset_bytes(host)
    before = sorted(p.name for p in tmp_path.iterdir())
    messages = []
    for route in ("host", None):
        if route:
            monkeypatch.setenv("SAI_AMD_INGEST", route)
        else:
            monkeypatch.delenv("SAI_AMD_INGEST")
        with pytest.raises(ValueError, match=r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2: a .geno record holds") as refusal:
            convert(case["vcf"], "7", out_eigenstrat=str(tmp_path / "refused"), geno_format=fmt)
        messages.append(str(refusal.value))
        assert sorted(p.name for p in tmp_path.iterdir()) == before
    assert messages[0] == messages[1]  # the same sample and position


# ---- score on the converted fileset ----


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_the_converted_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc, fmt):
    from sai_amd.sai import convert

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    prefix = str(tmp_path / "fx")
    convert(vcf, chrom, out_eigenstrat=prefix, geno_format=fmt)
    # with and without ancestral alleles; Danc and Dplus of the outgroup fixture are refused without them
    for k, anc_file in enumerate([anc, None] if anc and "outgroup" not in cfgfile else [anc]):
        want = score_files(vcf, chrom, cfgfile, anc_file, tmp_path / f"vcf{k}" / "s.tsv")
        assert score_files(prefix + ".geno", chrom, cfgfile, anc_file, tmp_path / f"set{k}" / "s.tsv") == want and len(want[".tsv"].splitlines()) > 1
