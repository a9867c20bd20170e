"""The host routes (``SAI_AMD_INGEST=host``: ``load_dosage(..., buffer_bytes=cap)`` over ``read_batches``) of every
streaming reader at a sweep of buffer sizes that puts a batch boundary before and behind every selected row
(tests/batch_sweep_cases.py), against the block the matrix says, byte for byte; and the two ``convert`` writers at
every batch size against their one-batch files."""

import numpy as np
import pytest

import batch_sweep_cases as S


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return S.write_all(tmp_path_factory.mktemp("sweep"))


def fileset_route(kind: str):
    """(reader module, key of the fileset in ``files``, variants of chromosome 7 in it)."""
    from sai_amd.utils import eigenstrat, pgen, plink

    return {"bed": (plink, "bed", 60), "pgen": (pgen, "pgen", 60), "text": (eigenstrat, "text", 60), "text_open": (eigenstrat, "text_open", 60),
            "packed": (eigenstrat, "packed", 60), "transposed": (eigenstrat, "transposed", S.N_LONG)}[kind]  # fmt: skip


def host_index(reader, prefix, req, anc):
    ffi = {"plink": "_ffi_plink", "pgen": "_ffi_pgen", "eigenstrat": "_ffi_eigenstrat"}[reader.__name__.rsplit(".", 1)[1]]
    return reader._Index(getattr(reader, ffi).load_host(), prefix, S.CHROM, req.names, req.ploidies, req.start, req.end, anc, 2)


def check_cover(kind, name, sweep, n_rows):
    """The cover conditions of the sweep: they are conditions on the case data, not on the code."""
    assert sweep.firsts == set(range(n_rows)) and sweep.lasts == set(range(n_rows))  # a boundary before and behind every selected row
    assert sweep.most >= 4 and sweep.several >= 3  # three batches and more at several caps: both buffers are used again
    if name == "sparse" and kind in ("bed", "text", "text_open", "packed"):
        assert sweep.empty > 0  # the row planner: a batch of read-through rows only


@pytest.mark.parametrize("name", S.REQUESTS)
@pytest.mark.parametrize("kind", ["bed", "pgen", "text", "text_open", "packed", "transposed"])
def test_fileset_host_route_at_every_batch_boundary(files, kind, name):
    reader, key, n_here = fileset_route(kind)
    req = S.request(name, n_here=n_here)
    anc = (files["anc"] if n_here == 60 else files["anc_long"]) if req.anc else None
    want = S.expected(name, n_here=n_here)
    idx = host_index(reader, files[key], req, anc)
    assert idx.pos.tolist() == want[0].tolist() and idx.flip.tolist() == S.selection(name, n_here)[1].tolist()  # the index selects what the matrix says
    sweep = S.cap_sweep(idx.batches)
    if kind == "transposed":  # a batch is a range of variants at a stride of whole words: its boundaries fall where the stride puts them
        assert sweep.most >= 4 and sweep.several >= 3 and {b.first_code for cap in sweep.caps for b in idx.batches(cap)} == {0, 1, 2, 3}
    else:
        check_cover(kind, name, sweep, len(want[0]))
    with pytest.raises(ValueError, match=f"^SAI_AMD_INGEST_BUFFER of {sweep.refused} bytes is smaller than one "):
        reader.load_dosage(files[key], S.CHROM, req.names, req.ploidies, req.start, req.end, anc, buffer_bytes=sweep.refused)
    assert len(sweep.caps) <= 160
    for cap in sweep.caps:
        pos, dos, n_matched, n_anc = reader.load_dosage(files[key], S.CHROM, req.names, req.ploidies, req.start, req.end, anc, buffer_bytes=cap)
        assert pos.dtype == np.int32 and pos.tolist() == want[0].tolist() and (n_matched, n_anc) == want[2:], (kind, name, cap)
        assert dos.dtype == np.int8 and dos.shape == want[1].shape and np.array_equal(dos, want[1]), (kind, name, cap, sweep.plans[cap])


def test_the_two_statements_of_the_block_agree():
    """The dosage table of the filesets and the allele rule of VCF text and BCF give the same block wherever both
    apply (ploidies 1 and 2, no heterozygous call in a haploid slot)."""
    m = S.matrix()
    for name in S.REQUESTS:
        req = S.request(name)
        rows, flips, _, _ = S.selection(name)
        assert np.array_equal(S.expected_vcf(m.codes[rows], req.cols, req.ploidies, flips), S.expected(name)[1])
    wide = S.request("general", wide=True)
    assert set(wide.ploidies) == {1, 2, 3, 4} and len(set(wide.names)) == 19


def bcf_sizes(path, req, anc):
    """The bytes of the GT array of every selected row, from one batch of the host stream."""
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    cap = 1 << 20
    bufs = [np.empty(cap, dtype=np.uint8) for _ in range(2)]
    with bcf._Stream(_ffi_bcf.load_host(), path, S.CHROM, req.names, req.ploidies, req.start, req.end, anc, 2, [b.ctypes.data for b in bufs], cap) as stream:
        _, _, pos, _, off, width, length = stream.next()
        assert stream.next() is None
        return [int(w) * int(n) * stream.n_cols for w, n in zip(width, length)], pos


def bcf_batch_rows(path, req, anc, cap):
    """Rows per batch of the host stream at ``cap``."""
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    bufs = [np.empty(cap, dtype=np.uint8) for _ in range(2)]
    out = []
    with bcf._Stream(_ffi_bcf.load_host(), path, S.CHROM, req.names, req.ploidies, req.start, req.end, anc, 2, [b.ctypes.data for b in bufs], cap) as stream:
        while True:
            got = stream.next()
            if got is None:
                return out
            out.append(len(got[2]))


@pytest.mark.parametrize("name", S.REQUESTS)
def test_bcf_host_route_at_every_batch_boundary(files, name):
    from sai_amd import _ffi_bcf
    from sai_amd.utils import bcf

    req = S.request(name, wide=True)
    anc = files["anc"] if req.anc else None
    want = S.expected(name, wide=True)
    sizes, pos = bcf_sizes(files["bcf"], req, anc)
    assert pos.tolist() == want[0].tolist() and set(sizes) == {2 * S.N_IND}
    sweep = S.cap_sweep(lambda cap: S.bcf_plan(sizes, cap, _ffi_bcf.SAI_BCF_GT_ALIGN))
    check_cover("bcf", name, sweep, len(want[0]))
    with pytest.raises(ValueError, match=f"the staging buffer of {sweep.refused} bytes is smaller than the GT array of record 7:{want[0][0]} "):
        bcf.load_dosage(files["bcf"], S.CHROM, req.names, req.ploidies, req.start, req.end, anc, buffer_bytes=sweep.refused)
    for cap in sweep.caps:
        assert bcf_batch_rows(files["bcf"], req, anc, cap) == [k1 - k0 for k0, k1 in sweep.plans[cap]], cap  # the restated plan is the stream's
        pos, dos, n_matched, n_anc = bcf.load_dosage(files["bcf"], S.CHROM, req.names, req.ploidies, req.start, req.end, anc, buffer_bytes=cap)
        assert pos.tolist() == want[0].tolist() and (n_matched, n_anc) == want[2:], (name, cap)
        assert dos.dtype == np.int8 and np.array_equal(dos, want[1]), (name, cap)


def convert_sweep(convert, extensions, vcf, folder, monkeypatch, every: bool, want=None):
    """``convert`` with SAI_AMD_CONVERT_BATCH set for 1, 2, 3, ... rows per batch, up to all rows plus one, against the
    one-batch files.  The writers round a batch down to a multiple of 16 rows (at least 16): with ``every`` unset only
    the sizes at which that number changes are run.  ``want`` = the files another route wrote, which the one-batch files
    must equal too.  -> the rows per batch that occurred"""
    from sai_amd.utils import bed_writer

    haploid = [S.SAMPLES[c] for c in S.HAPLOID_COLS]
    row_bytes = (S.N_IND + 3) // 4
    monkeypatch.delenv("SAI_AMD_CONVERT_BATCH", raising=False)
    done = convert(vcf, S.CHROM, str(folder / "one"), haploid_samples=haploid)
    assert done["rows_written"] == S.N_LONG
    one = {ext: (folder / f"one{ext}").read_bytes() for ext in extensions}
    assert want is None or one == want
    want = one
    steps, before = [], None
    for rows in range(1, S.N_LONG + 2):
        monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", str(rows * row_bytes))
        step = bed_writer._batch_rows(row_bytes)
        if every or step != before or rows == S.N_LONG + 1:
            convert(vcf, S.CHROM, str(folder / "cut"), haploid_samples=haploid)
            assert {ext: (folder / f"cut{ext}").read_bytes() for ext in extensions} == want, rows
            for ext in extensions:
                (folder / f"cut{ext}").unlink()
        if step != before:
            steps.append(step)
        before = step
    monkeypatch.delenv("SAI_AMD_CONVERT_BATCH")
    return steps


@pytest.mark.parametrize("fileset", ["bfile", "pfile"])
def test_convert_host_route_at_every_batch_size(files, tmp_path, monkeypatch, fileset):
    from sai_amd.utils import bed_writer, pgen_writer

    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    convert, extensions = {"bfile": (bed_writer.convert, (".bed", ".bim", ".fam")), "pfile": (pgen_writer.convert, (".pgen", ".pvar", ".psam"))}[fileset]
    steps = convert_sweep(convert, extensions, files["vcf_long"], tmp_path, monkeypatch, every=True)
    assert steps == list(range(16, (S.N_LONG + 1) // 16 * 16 + 1, 16))  # 16 rows a batch (twenty-five batches) to 400 (one)
