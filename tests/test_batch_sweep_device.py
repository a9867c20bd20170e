"""Every streaming reader on the GPU at a sweep of buffer sizes that puts a batch boundary before and behind every
selected row (tests/batch_sweep_cases.py): the kernels are called with whatever ``out_row0`` the planners produce, the
third and later batches reuse a pinned buffer, a batch of the row planner may hold no selected row, a ``.pgen`` batch
may open with a difference row whose base is fetched again, and a transposed ``.geno`` batch starts at each of the four
positions in a byte.  Every read is compared, byte for byte, with the block the matrix says; the one-batch host read
is the second witness.  Every input is a valid file."""

import functools

import numpy as np
import pytest

import batch_sweep_cases as S
import bcf_builder
from test_batch_sweep_cpu import bcf_sizes, check_cover, convert_sweep, fileset_route, host_index
from test_bed_pack2_cpu import pack_numpy

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


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return S.write_all(tmp_path_factory.mktemp("sweep"))


def same_read(got, want, where):
    pos, dos, n_matched, n_anc = got
    assert pos.dtype == np.int32 and pos.tolist() == want[0].tolist() and (n_matched, n_anc) == tuple(want[2:]), where
    host = dos.cpu().numpy() if hasattr(dos, "cpu") else dos
    assert host.dtype == np.int8 and host.shape == want[1].shape and np.array_equal(host, want[1]), where


@pytest.mark.parametrize("name", S.REQUESTS)
@pytest.mark.parametrize("kind", ["bed", "pgen", "text", "text_open", "packed", "transposed"])
def test_fileset_reader_at_every_batch_boundary(eng, files, kind, name):
    reader, key, n_here = fileset_route(kind)
    req = S.request(name, n_here=n_here)
    anc = (files["anc"] if n_here == 60 else files["anc_long"]) if req.anc else None
    want = S.expected(name, n_here=n_here)
    ask = (files[key], S.CHROM, req.names, req.ploidies, req.start, req.end, anc)
    same_read(reader.load_dosage(*ask), want, (kind, name, "host"))
    idx = host_index(reader, files[key], req, anc)
    sweep = S.cap_sweep(idx.batches)
    if kind == "transposed":
        assert sweep.most >= 4 and sweep.several >= 3 and {b.first_code for cap in sweep.caps for b in idx.batches(cap)} == {0, 1, 2, 3}
    else:
        check_cover(kind, name, sweep, len(want[0]))
    with pytest.raises(ValueError, match=f"^SAI_AMD_INGEST_BUFFER of {sweep.refused} bytes is smaller than one "):
        reader.load_dosage_device(eng, *ask, buffer_bytes=sweep.refused)
    for cap in sweep.caps:
        same_read(reader.load_dosage_device(eng, *ask, buffer_bytes=cap), want, (kind, name, cap, sweep.plans[cap]))
    reader.release_buffers(eng)


def populations_of(req):
    """The slots of a request as populations of one ploidy each: [(slots, ploidy)], a repeated sample in two of them."""
    two = [k for k, p in enumerate(req.ploidies) if p == 2]
    one = [k for k, p in enumerate(req.ploidies) if p == 1]
    parts = [(two, 2)] if not one else [(two[0::2], 2), (two[1::2], 2), (one, 1)]
    assert all(len({req.names[k] for k in slots}) == len(slots) for slots, _ in parts)
    return parts


@pytest.mark.parametrize("name", S.REQUESTS)
@pytest.mark.parametrize("kind", ["bed", "pgen"])
def test_packed2_reader_at_every_batch_boundary(eng, files, kind, name):
    """The same sweep into the 2-bit layout: one ``pack2`` call per population and batch, a site's words shared between
    the batches that meet inside a tile of 64 sites."""
    reader, key, _ = fileset_route(kind)
    req = S.request(name)
    anc = files["anc"] if req.anc else None
    pos_want, block, n_matched, n_anc = S.expected(name)
    parts = populations_of(req)
    pops = [([req.names[k] for k in slots], ploidy) for slots, ploidy in parts]
    want = [pack_numpy(np.where(block[:, slots] < 0, 3, block[:, slots]).astype(np.uint8)) for slots, _ in parts]
    assert int(block.max()) <= 2  # the case data: no missing call in a flipped row of these columns
    flat = S.request(name)
    flat.names, flat.ploidies = [n for names, _ in pops for n in names], [p for names, p in pops for _ in names]
    sweep = S.cap_sweep(host_index(reader, files[key], flat, anc).batches)
    check_cover(kind, name, sweep, len(pos_want))
    ask = (files[key], S.CHROM, pops, req.start, req.end, anc)
    host = reader.load_packed(*ask)
    assert all(np.array_equal(h, w) for h, w in zip(host[1], want)) and host[0].tolist() == pos_want.tolist()
    for cap in sweep.caps:
        pos, packed, got_matched, got_anc = reader.load_packed_device(eng, *ask, buffer_bytes=cap)
        assert pos.tolist() == pos_want.tolist() and (got_matched, got_anc) == (n_matched, n_anc), (kind, name, cap)
        for p, (got, w) in enumerate(zip(packed, want)):
            assert (got.n_sites, got.n_ind) == (len(pos_want), len(parts[p][0]))
            assert np.array_equal(got.data.cpu().numpy(), w), (kind, name, cap, p, sweep.plans[cap])
    reader.release_buffers(eng)


@pytest.mark.parametrize("name", S.REQUESTS)
def test_bcf_host_walk_route_at_every_batch_boundary(eng, files, monkeypatch, name):
    """``SAI_AMD_GPU_INFLATE=0``: the host walks the records and a batch is as many GT arrays as fit the buffer."""
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    monkeypatch.setenv("SAI_AMD_GPU_INFLATE", "0")
    req = S.request(name, wide=True)
    anc = files["anc"] if req.anc else None
    want = S.expected(name, wide=True)
    ask = (files["bcf"], S.CHROM, req.names, req.ploidies, req.start, req.end, anc)
    same_read(bcf.load_dosage(*ask), want, (name, "host"))
    sizes, _ = bcf_sizes(files["bcf"], req, anc)
    sweep = S.cap_sweep(lambda cap: S.bcf_plan(sizes, cap, _ffi_bcf.SAI_BCF_GT_ALIGN))
    check_cover("bcf", name, sweep, len(want[0]))
    for k, cap in enumerate(sweep.caps):
        trace = {}
        if k % 2:
            monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", str(cap))
            got = bcf.load_dosage_device(eng, *ask, trace=trace)
            monkeypatch.delenv("SAI_AMD_INGEST_BUFFER")
        else:
            got = bcf.load_dosage_device(eng, *ask, buffer_bytes=cap, trace=trace)
        assert trace["route"] == "host"
        same_read(got, want, (name, cap, sweep.plans[cap]))
    bcf.release_buffers(eng)


@pytest.mark.parametrize("name", S.REQUESTS)
def test_bcf_gpu_walk_route_at_every_member_boundary(eng, files, monkeypatch, name):
    """Members of 300 inflated bytes and ``SAI_AMD_INFLATE_BATCH`` at every value at which the members of a batch
    change: records straddle members and batches, and what is carried in front of the next batch has every length."""
    from sai_amd.utils import bcf

    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    req = S.request(name, wide=True)
    anc = files["anc"] if req.anc else None
    want = S.expected(name, wide=True)
    ask = (files["bcf"], S.CHROM, req.names, req.ploidies, req.start, req.end, anc)
    n_stream = len(bcf_builder.inflated_stream(S.vcf_text()))
    sizes = [min(300, n_stream - at) for at in range(0, n_stream, 300)]
    sweep = S.cap_sweep(lambda cap: S.member_plan(sizes, cap), start=300)
    assert sweep.most == len(sizes) >= 25 and sweep.several >= 3
    assert sweep.firsts == set(range(len(sizes))) and sweep.lasts == set(range(len(sizes)))  # a batch ends behind every member
    for cap in sweep.caps:
        monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", str(cap))
        trace = {}
        got = bcf.load_dosage_device(eng, *ask, trace=trace)
        assert trace["route"] == "device", cap
        same_read(got, want, (name, cap))
    bcf.release_buffers(eng)


def record_lines(text: str, newline: str):
    """(offset of the first record line, [(offset, length with its newline)] of every record line)."""
    at, out = 0, []
    for line in text.split(newline)[:-1]:
        if not line.startswith("#"):
            out.append((at, len(line) + len(newline)))
        at += len(line) + len(newline)
    return out[0][0], out


@pytest.mark.parametrize("name", S.REQUESTS)
@pytest.mark.parametrize("newline", ["lf", "crlf"])
def test_vcf_text_with_a_batch_boundary_at_every_byte_of_two_lines(eng, tmp_path, monkeypatch, newline, name):
    """Plain text: a batch is ``SAI_AMD_INGEST_BUFFER`` bytes (64 KiB at least) from where the last one ended, cut back
    to a line end.  The first batch's raw end falls at every byte of two record lines of the chromosome (the byte behind
    their newline included); the later batches' ends fall wherever the lines' lengths put them."""
    from sai_amd.utils import native_vcf
    from sai_amd.utils.device_vcf import load_dosage_device

    nl = "\n" if newline == "lf" else "\r\n"
    text = S.vcf_text(S.N_BGZIP, nl)
    path = S.write_text(tmp_path / "m.vcf", text)
    data_off, lines = record_lines(text, nl)
    req = S.request(name, wide=True, n_here=S.N_BGZIP)
    anc = S.write_anc(tmp_path / "anc.bed", S.N_BGZIP) if req.anc else None
    want = S.expected(name, wide=True, n_here=S.N_BGZIP)
    ask = (path, S.CHROM, req.names, req.ploidies, req.start, req.end, anc)
    same_read(native_vcf.load_dosage(*ask), want, (name, "host"))
    first = next(k for k, (off, _) in enumerate(lines) if off - data_off >= 1 << 16)  # the first line a batch of 64 KiB can end in
    caps = [off - data_off + j for off, n in (lines[first], lines[first + 9]) for j in range(n + 1)]
    assert min(caps) >= 1 << 16 and len(text) - data_off > 2 * max(caps)  # three batches at every cap
    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    for cap in caps:
        monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", str(cap))
        same_read(load_dosage_device(eng, *ask), want, (name, newline, cap))
    monkeypatch.delenv("SAI_AMD_INGEST_BUFFER")
    eng.release_ingest_buffers()


@functools.lru_cache(maxsize=None)
def member_sweep(sizes):
    """The sweep of ``SAI_AMD_INFLATE_BATCH`` of a bgzip VCF with members of ``sizes`` inflated bytes, from the 64 KiB the
    route asks for at least."""
    return S.cap_sweep(lambda cap: S.member_plan(sizes, cap), start=1 << 16)


@pytest.mark.parametrize("name", S.REQUESTS)
@pytest.mark.parametrize("newline", ["lf", "crlf"])
def test_bgzip_vcf_with_a_batch_boundary_between_every_pair_of_members(eng, tmp_path, monkeypatch, newline, name):
    """bgzip: a batch is as many whole members as inflate to at most ``SAI_AMD_INFLATE_BATCH`` bytes, 64 KiB at least.
    The first member is a full one of meta lines, the others hold 1 000 bytes: the sweep ends a batch behind every
    member, lines straddle members and batches, and the record text fills three batches."""
    from sai_amd.utils import native_vcf
    from sai_amd.utils.device_vcf import load_dosage_device

    nl = "\n" if newline == "lf" else "\r\n"
    text = S.bgzip_text(nl)
    path, sizes = S.write_bgzip(tmp_path / "m.vcf.gz", text, S.BGZIP_MEMBER, S.BGZIP_FIRST)
    req = S.request(name, wide=True, n_here=S.N_BGZIP)
    anc = S.write_anc(tmp_path / "anc.bed", S.N_BGZIP) if req.anc else None
    want = S.expected(name, wide=True, n_here=S.N_BGZIP)
    ask = (path, S.CHROM, req.names, req.ploidies, req.start, req.end, anc)
    same_read(native_vcf.load_dosage(*ask), want, (name, "host"))

    sweep = member_sweep(tuple(sizes))
    ends = {k1 for batches in sweep.plans.values() for _, k1 in batches}
    assert ends == set(range(1, len(sizes) + 1)) and sweep.most >= 3 and sweep.several >= 3  # a batch ends behind every member
    monkeypatch.delenv("SAI_AMD_GPU_INFLATE", raising=False)
    for k, cap in enumerate(sweep.caps):
        if k % 2:
            monkeypatch.setenv("SAI_AMD_INFLATE_BATCH", str(cap))
            got = load_dosage_device(eng, *ask)
            monkeypatch.delenv("SAI_AMD_INFLATE_BATCH")
        else:
            got = load_dosage_device(eng, *ask, buffer_bytes=cap)
        same_read(got, want, (name, newline, cap))
        assert eng.__dict__["_inflate_state"]["last"]["members"] >= len(sizes)  # the members were inflated on the GPU
    eng.release_ingest_buffers()


@pytest.mark.parametrize("fileset", ["bfile", "pfile"])
def test_convert_gpu_route_at_every_batch_size(eng, files, tmp_path, monkeypatch, fileset):
    """The encoders write a batch into one of two pinned buffers in turn: every number of rows per batch the writers
    can take (multiples of 16), against the files of the host route."""
    from sai_amd.utils import bed_writer, pgen_writer

    convert, extensions = {"bfile": (bed_writer.convert, (".bed", ".bim", ".fam")), "pfile": (pgen_writer.convert, (".pgen", ".pvar", ".psam"))}[fileset]
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    monkeypatch.delenv("SAI_AMD_CONVERT_BATCH", raising=False)
    haploid = [S.SAMPLES[c] for c in S.HAPLOID_COLS]
    (tmp_path / "host").mkdir()
    convert(files["vcf_long"], S.CHROM, str(tmp_path / "host" / "one"), haploid_samples=haploid)
    want = {ext: (tmp_path / "host" / f"one{ext}").read_bytes() for ext in extensions}
    monkeypatch.delenv("SAI_AMD_INGEST")
    steps = convert_sweep(convert, extensions, files["vcf_long"], tmp_path, monkeypatch, every=False, want=want)
    assert steps == list(range(16, (S.N_LONG + 1) // 16 * 16 + 1, 16))
