"""The BCF route that finds the records on the GPU, on the GPU: ``sai_bcf_chain_segments`` and ``sai_bcf_record_heads``
against their host twins bit for bit on the streams of tests/test_bcf_walk_cpu.py, ``load_dosage_device`` through the
GPU route against the host route and the host reader, the damaged files, the scan, and ``score``."""

import ctypes as C
import re

import numpy as np
import pytest

import bcf_builder as B
from test_bcf_cpu import FILES, REFUSED, anc_file, region_of, samples_of, small_bcf, vcf_text
from test_bcf_walk_cpu import DENSE, SHAPES, Stream, decoy_stream, host_heads, host_kernels, one_sample_vcf, walk

pytestmark = pytest.mark.gpu

GUARD = 256


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


def device_functions(eng):
    """(kernels, heads_of) for ``walk``: the two kernels, their text between guard bytes that must stay as they are."""
    import torch

    from sai_amd import _ffi, _ffi_bcf_device as D

    lib = D.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def guarded(data):
        whole = np.concatenate([np.full(GUARD, 0xA5, np.uint8), data, np.full(GUARD, 0xA5, np.uint8)])
        return whole, torch.from_numpy(whole).to(eng.device)

    def kernels(data, n_bytes, seg_bytes, max_heads, st):
        whole, d_text = guarded(data)
        n_seg = -(-n_bytes // seg_bytes)
        d_chains = torch.full((n_seg * max_heads * 16 + 16,), 0x5A, dtype=torch.uint8, device=eng.device)
        d_info = torch.full((n_seg + 1,), -7, dtype=torch.int32, device=eng.device)
        d_contigs = torch.from_numpy(st.contig_defined).to(eng.device)
        _ffi.check(lib.sai_bcf_chain_segments(eng.ctx, C.c_void_p(d_text.data_ptr() + GUARD), n_bytes, seg_bytes, max_heads, p(d_contigs),
                                              len(st.contig_defined), st.n_sample, p(d_chains), p(d_info), stream))  # fmt: skip
        torch.cuda.synchronize()
        chains, info = d_chains.cpu().numpy(), d_info.cpu().numpy()
        assert np.array_equal(d_text.cpu().numpy(), whole) and (chains[-16:] == 0x5A).all() and info[-1] == -7
        return chains[:-16].view(D.CHAIN).copy(), info[:-1].copy()

    def heads_of(data, n_bytes, seg_bytes, seg_entry, seg_first, carry_from, n_records, gt_key, want_gt):
        whole, d_text = guarded(data)
        d_heads = torch.full(((n_records + 1) * 64,), 0x5A, dtype=torch.uint8, device=eng.device)
        d_entry, d_first = torch.from_numpy(seg_entry).to(eng.device), torch.from_numpy(seg_first).to(eng.device)
        _ffi.check(lib.sai_bcf_record_heads(eng.ctx, C.c_void_p(d_text.data_ptr() + GUARD), n_bytes, seg_bytes, p(d_entry), p(d_first), carry_from,
                                            n_records, gt_key, int(want_gt), p(d_heads), stream))  # fmt: skip
        torch.cuda.synchronize()
        heads = d_heads.cpu().numpy()
        assert np.array_equal(d_text.cpu().numpy(), whole) and (heads[-64:] == 0x5A).all()
        return heads[:-64].view(D.HEAD).copy()

    return kernels, heads_of


def streams():
    """(name, stream, bytes of the batch or None for all of them, e0 or None): the cases of the CPU tests."""
    out = [(f"example {shape}", Stream(vcf_text("example.vcf"), **shape), None, None) for shape in SHAPES]
    out.append(("seeded", Stream(vcf_text("seeded"), width=2, extra_before=True, extra_after=True), None, None))
    for pad in (0, 3, 17, 40, 77):  # record starts around a boundary of 256 bytes
        out.append((f"boundary {pad}", Stream(one_sample_vcf(12, id_of=lambda k, pad=pad: "x" * pad if k == 3 else "")), None, None))
    out.append(("long records", Stream(one_sample_vcf(9, samples=[f"s{k}" for k in range(700)])), None, None))
    out.append(("short records", Stream(one_sample_vcf(400)), None, None))
    out.append(("decoys", decoy_stream(align=5)[1], None, None))
    out.append(("decoys behind GT", decoy_stream(last=True)[1], None, None))
    out.append(("dense", decoy_stream(n_copies=10, gap=1)[1], None, None))
    for damage in (dict(l_indiv=77), dict(n_sample=10), dict(chrom=5), dict(l_shared=23)):
        out.append((f"broken {damage}", Stream(vcf_text("example.vcf"), on_record=lambda i, r, damage=damage: i == 6 and r.update(damage)), None, None))
    st = Stream(vcf_text("example.vcf"), width=2)
    for cut in (st.records[5]["off"] + 7, st.records[9]["off"] + 31, st.records[9]["off"] + 33, st.data_off, st.data_off + 1):
        out.append((f"cut at {cut}", st, st.bytes[:cut], None))
    out.append(("carry + rest", st, st.bytes[st.records[5]["off"] :], 0))
    return out


@pytest.mark.parametrize("seg_bytes", [256, 16384])
def test_the_kernels_equal_their_host_twins(eng, seg_bytes):
    kernels, heads_of = device_functions(eng)
    verdicts, dense, partial = set(), False, False
    for name, st, data, e0 in streams():
        for want_gt in (True, False):
            host = walk(st, seg_bytes, data=data, e0=e0, want_gt=want_gt, kernels=host_kernels, heads_of=host_heads)
            dev = walk(st, seg_bytes, data=data, e0=e0, want_gt=want_gt, kernels=kernels, heads_of=heads_of)
            assert dev["chains"].tobytes() == host["chains"].tobytes() and np.array_equal(dev["info"], host["info"]), (name, seg_bytes)
            assert (dev["verdict"], dev["n_records"], dev["carry_from"]) == (host["verdict"], host["n_records"], host["carry_from"]), (name, seg_bytes)
            if host["verdict"] == 0:
                assert dev["heads"].tobytes() == host["heads"].tobytes(), (name, seg_bytes, want_gt)
            verdicts.add(host["verdict"])
            dense |= bool((host["info"] & DENSE).any())
            partial |= len(host["data"]) % seg_bytes != 0
    assert verdicts == {0, 1} and partial and (dense or seg_bytes == 256)
    # more heads than the default, and a batch of more than one tile of 16 KiB per segment
    st = decoy_stream(n_copies=10, gap=1)[1]
    for max_heads in (1, 8, 64):
        host, dev = (walk(st, 1024, max_heads=max_heads, kernels=k, heads_of=h) for k, h in ((host_kernels, host_heads), (kernels, heads_of)))
        assert dev["chains"].tobytes() == host["chains"].tobytes() and np.array_equal(dev["info"], host["info"]) and dev["verdict"] == host["verdict"]
        assert bool((host["info"] & DENSE).any()) == (max_heads < 64) and host["verdict"] == (max_heads < 64)
    st = Stream(one_sample_vcf(2500))
    assert len(st.bytes) > 65536 + 16384
    host, dev = (walk(st, 65536, kernels=k, heads_of=h) for k, h in ((host_kernels, host_heads), (kernels, heads_of)))
    assert host["verdict"] == 0 and host["n_records"] == 2500
    assert dev["chains"].tobytes() == host["chains"].tobytes() and np.array_equal(dev["info"], host["info"]) and dev["heads"].tobytes() == host["heads"].tobytes()


def equal_reads(a, b) -> bool:
    return a[0].tolist() == b[0].tolist() and np.array_equal(np.asarray(a[1].cpu() if hasattr(a[1], "cpu") else a[1]), np.asarray(b[1].cpu() if hasattr(b[1], "cpu") else b[1])) \
        and tuple(a[2:]) == tuple(b[2:])  # fmt: skip


@pytest.mark.parametrize("name,chrom,given_anc", [FILES[0], FILES[3], FILES[4]], ids=[FILES[0][0], FILES[3][0], FILES[4][0]])
def test_load_dosage_device_through_the_gpu_route(eng, tmp_path, monkeypatch, name, chrom, given_anc):
    """Members of 300 bytes and batches of a few KiB: records straddle members and batches, the carry is used.  With and
    without the EOF member, a chromosome the file does not hold, a region with ancestral alleles."""
    from sai_amd.utils import bcf

    samples = samples_of(name)
    anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
    batch = 4096 if len(samples) < 100 else 40000
    requests = [(samples, [2] * len(samples)), (samples[::-1][:-1], [1 + k % 4 for k in range(len(samples) - 1)])]
    for k, shape in enumerate((dict(width=1, member_size=300), dict(width=2, idx=True, extra_before=True, extra_after=True, member_size=300, eof=False))):
        path = B.write_bcf(tmp_path / f"{k}.bcf", vcf_text(name), **shape)
        for names, ploidies in requests:
            for a, (start, end), ask_chrom in ((None, (None, None), chrom), (anc, region, chrom), (None, (None, None), "nope")):
                monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", str(batch))
                monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
                trace = {}
                got = bcf.load_dosage_device(eng, path, ask_chrom, names, ploidies, start, end, a, trace=trace)
                assert trace["route"] == "device", (shape, a, ask_chrom)
                monkeypatch.setenv("SAI_AMD_GPU_INFLATE", "0")
                trace = {}
                host_route = bcf.load_dosage_device(eng, path, ask_chrom, names, ploidies, start, end, a, trace=trace)
                assert trace["route"] == "host"
                want = bcf.load_dosage(path, ask_chrom, names, ploidies, start, end, a)
                assert equal_reads(got, want) and equal_reads(host_route, want), (shape, a, ask_chrom)
                assert len(want[0]) > 0 or ask_chrom == "nope"
    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", "300")
    if len(samples) > 100:
        with pytest.raises(ValueError, match="a record does not fit a batch of 300 inflated bytes: raise SAI_AMD_INFLATE_BATCH"):
            bcf.load_dosage_device(eng, path, chrom, samples, [2] * len(samples))
    bcf.release_buffers(eng)


def test_damaged_files_raise_the_host_routes_sentence(eng, tmp_path, monkeypatch):
    from sai_amd.utils import bcf

    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", "4096")
    samples = samples_of("example.vcf")
    for name, options, sentence in REFUSED:
        path = small_bcf(tmp_path, name + ".bcf", **options)
        trace = {}
        with pytest.raises(ValueError, match=re.escape(path) + ".*" + sentence):
            bcf.load_dosage_device(eng, path, "21", samples, [2] * len(samples), trace=trace)
        assert trace["route"] == "host", name
    bcf.release_buffers(eng)


def test_the_scan_on_the_device_equals_the_host_scan(eng, tmp_path, monkeypatch):
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    monkeypatch.delenv("SAI_AMD_INGEST", raising=False)
    monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", "4096")
    lib = _ffi_bcf.load_host()
    path = B.write_bcf(tmp_path / "seeded.bcf", vcf_text("seeded"), member_size=300, width=2)
    for chrom in ("7", "3", "9", "nope", ""):
        v = [C.c_int64(-1) for _ in range(4)]
        assert lib.sai_bcf_scan(path.encode(), chrom.encode(), *[C.byref(x) for x in v]) == 0
        want = tuple(x.value for x in v)
        assert bcf._scan_on_device(path, chrom) == want, chrom
        bcf._scanned.clear()
        assert bcf.scan_first_last(path, chrom) == ((None, None) if want[0] < 0 else want[:2]) and bcf.header_counts(path) == want[2:]
    bcf._scanned.clear()
    damaged = small_bcf(tmp_path, "l_shared.bcf", on_record=lambda i, r: i == 1 and r.update(l_shared=23))
    assert bcf._scan_on_device(damaged, "21") is None
    with pytest.raises(ValueError, match="record 2 has l_shared = 23"):
        bcf.scan_first_last(damaged, "21")
    bcf.release_buffers(eng)


def test_score_on_a_bcf_is_the_same_on_both_routes(eng, in_repo_root, tmp_path, monkeypatch):
    from test_bcf_device import score_files

    from sai_amd.utils import bcf

    vcf, chrom, cfgfile, anc = "tests/data/test.mixed.ploidy.data.vcf.gz", "21", "tests/data/test_mixed_ploidy.config.yaml", "tests/data/test.mixed.ploidy.data.anc.alleles"
    path = B.write_bcf(tmp_path / "calls.bcf", B.read_vcf_text(vcf), width=2, idx=True, extra_before=True, member_size=977, eof=False)
    monkeypatch.setenv("SAI_AMD_INGEST", "device")
    monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", "20000")
    monkeypatch.setenv("SAI_AMD_GPU_INFLATE", "0")
    want = score_files(path, chrom, cfgfile, anc, tmp_path / "host" / "s.tsv")
    assert set(want) >= {".tsv"} and len(want[".tsv"].splitlines()) > 1
    monkeypatch.delenv("SAI_AMD_GPU_INFLATE")
    bcf._scanned.clear()
    served = []  # a call that hands the read over raises and leaves nothing here
    real = bcf._load_device_walk

    def counted(*a, **k):
        got = real(*a, **k)
        served.append(len(got[0]))
        return got

    monkeypatch.setattr(bcf, "_load_device_walk", counted)
    assert score_files(path, chrom, cfgfile, anc, tmp_path / "device" / "s.tsv") == want
    assert served and max(served) > 0  # the GPU route returned rows to `score`, it did not hand them to the host route
