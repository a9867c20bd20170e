"""PLINK 1 ``.bed`` rows decoded straight into the packed2 layout, on the host: ``sai_bed_pack2_host`` against a numpy
statement of the layout formula of saihip.h and of the table of saihip_packed_ingest.h, the host reader
(``plink.load_packed``) and what ``score(..., layout="packed2")`` refuses before it reads anything."""

import ctypes as C
import numpy as np
import pytest

import abi_checks
import native_build
from conftest import ROOT
from test_plink_cpu import HET, HOM_A1, HOM_A2, MISSING, sai_cli, small_fileset

BAD_INDEX = 0x7FFFFFFF
# the table of saihip_packed_ingest.h by code 00, 01, 10, 11: a field, "het" (refused) or "unfit" (dosage 4)
TABLE = {(2, 0): [2, 3, 1, 0], (2, 1): [0, "unfit", 1, 2], (1, 0): [1, 3, "het", 0], (1, 1): [0, 2, "het", 1]}
N_IND = [1, 15, 16, 17, 48, 49, 63, 64, 65, 127, 128, 130]  # every w_tail 0..4, with zero, one and two full groups
N_SITES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def tile_words(n_ind):
    return (n_ind // 64) * 256 + ((n_ind % 64 + 15) // 16) * 64


def word_index(site, ind, n_ind):
    """saihip.h: the uint32 word that holds field (site, ind); the field is bits [2 * (ind % 16), +2) of it."""
    n_full, w_tail = n_ind // 64, (n_ind % 64 + 15) // 16
    full = (site // 64) * tile_words(n_ind) + (ind // 64) * 256 + (site % 64) * 4 + (ind % 64) // 16
    tail = (site // 64) * tile_words(n_ind) + n_full * 256 + (site % 64) * w_tail + (ind % 64) // 16
    return np.where(ind // 64 < n_full, full, tail)


def pack_numpy(fields, n_sites=None):
    """uint8 [sites][individuals] of 2-bit fields -> the block's bytes: padding individuals 0, padding sites all ones."""
    rows, n_ind = fields.shape
    n_sites = rows if n_sites is None else n_sites
    words = np.zeros(-(-n_sites // 64) * tile_words(n_ind), dtype=np.uint32)
    site, ind = np.arange(rows)[:, None], np.arange(n_ind)[None, :]
    np.bitwise_or.at(words, word_index(site, ind, n_ind), fields.astype(np.uint32) << (2 * (ind % 16)).astype(np.uint32))
    pad = np.arange(n_sites, -(-n_sites // 64) * 64)[:, None]
    if pad.size:
        words[word_index(pad, 16 * np.arange(-(-n_ind // 16))[None, :], n_ind)] = 0xFFFFFFFF
    return words.view(np.uint8)


def site_words(n_sites, n_ind, lo, hi):
    """Indices of the words of the sites [lo, hi) -- and of the padding sites when hi is the block's last site."""
    sites = np.arange(lo, -(-n_sites // 64) * 64 if hi == n_sites else hi)[:, None]
    return np.unique(word_index(sites, 16 * np.arange(-(-n_ind // 16))[None, :], n_ind))


def expect(rows, row_bytes, rib, flip, n_cols, cols, ploidy):
    """(fields [rows][individuals], status, unfit) from TABLE, cell by cell."""
    n_batch = len(rows) // row_bytes if row_bytes else 0
    n_ind = len(cols)
    fields = np.zeros((len(rib), n_ind), dtype=np.uint8)
    status, unfit = np.zeros(len(rib), dtype=np.int32), np.zeros(len(rib), dtype=np.int32)
    for r in range(len(rib)):
        for i in range(n_ind):
            col = int(cols[i])
            if not (0 <= rib[r] < n_batch and 0 <= col < n_cols):
                status[r] = BAD_INDEX
                continue
            code = (int(rows[int(rib[r]) * row_bytes + col // 4]) >> (2 * (col % 4))) & 3
            got = TABLE[(ploidy, int(flip[r] != 0))][code]
            if got == "het":
                status[r] = max(status[r], n_ind - i)
            elif got == "unfit":
                unfit[r] = max(unfit[r], n_ind - i)
            else:
                fields[r, i] = got
    return fields, status, unfit


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_host(rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, packed, n_sites, out_row0, n_threads=3):
    """One ``sai_bed_pack2_host`` call into ``packed``; returns (status, unfit)."""
    from sai_amd import _ffi, _ffi_packed_ingest

    lib = _ffi_packed_ingest.load_host()
    status, unfit = np.full(len(rib), -5, dtype=np.int32), np.full(len(rib), -5, dtype=np.int32)
    _ffi.check(lib.sai_bed_pack2_host(ptr(rows), len(rows) // row_bytes if row_bytes else 0, row_bytes, len(rib), ptr(rib), ptr(flip),
                                      n_cols, len(cols), None if first_col >= 0 else ptr(cols), first_col, ploidy, ptr(packed), n_sites,
                                      out_row0, ptr(status), ptr(unfit), n_threads), lib)  # fmt: skip
    return status, unfit


def column_lists(n_ind, n_cols, rng):
    """(first_col or -1, columns): a run at every first_col & 3, the same run without the promise, a permuted list with repeats."""
    out = [(f, np.arange(f, f + n_ind, dtype=np.int32)) for f in (0, 1, 2, 3)]
    out.append((-1, np.arange(5, 5 + n_ind, dtype=np.int32)))
    out.append((-1, rng.integers(0, n_cols, size=n_ind).astype(np.int32)))
    return out


def cuts_of(n_sites):
    """Calls cut at out_row0 = 0, 37 and 64: two calls complete the first tile."""
    edges = sorted({0, min(37, n_sites), min(64, n_sites), n_sites})
    return list(zip(edges, edges[1:]))


@pytest.mark.parametrize("n_ind", N_IND)
def test_host_decoder_equals_the_numpy_statement(n_ind):
    rng = np.random.default_rng(500 + n_ind)
    n_cols = n_ind + 9  # more columns than the run
    row_bytes = (n_cols + 3) // 4
    seen_het = seen_unfit = 0
    for n_sites in N_SITES:
        n_batch = n_sites + 3
        rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)  # any byte string is a valid row
        rib_all = rng.permutation(n_batch)[:n_sites].astype(np.int32)
        flip_all = rng.integers(0, 2, size=n_sites).astype(np.uint8)  # flipped and unflipped rows mixed
        for first_col, cols in column_lists(n_ind, n_cols, rng):
            for ploidy in (1, 2):
                fields, want_st, want_uf = expect(rows, row_bytes, rib_all, flip_all, n_cols, cols, ploidy)
                want = pack_numpy(fields)
                packed = np.full(want.size, 0xA5, dtype=np.uint8)
                written = np.zeros(want.size // 4, dtype=bool)
                for lo, hi in cuts_of(n_sites):
                    before = packed.copy()
                    st, uf = pack_host(rows, row_bytes, rib_all[lo:hi], flip_all[lo:hi], n_cols, cols, first_col, ploidy, packed, n_sites, lo)
                    assert np.array_equal(st, want_st[lo:hi]) and np.array_equal(uf, want_uf[lo:hi]), (n_ind, n_sites, first_col, ploidy, lo)
                    mine = np.zeros(want.size // 4, dtype=bool)
                    mine[site_words(n_sites, n_ind, lo, hi)] = True
                    assert np.array_equal(packed.view(np.uint32)[~mine], before.view(np.uint32)[~mine])  # nothing else is written
                    written |= mine
                assert written.all() and np.array_equal(packed, want), (n_ind, n_sites, first_col, ploidy)
                seen_het += int(want_st.any())
                seen_unfit += int(want_uf.any())
                assert not (want_st.any() and ploidy == 2) and not (want_uf.any() and ploidy == 1)
    assert seen_het and seen_unfit


def test_the_table_row_by_row_status_unfit_and_padding():
    rows = np.array([0b11100100, 0b11100100], dtype=np.uint8)  # per row: individuals 0..3 hold the codes 0, 1, 2, 3
    cols = np.arange(4, dtype=np.int32)
    for (ploidy, flipped), line in TABLE.items():
        for first_col in (0, -1):
            packed = np.full(tile_words(4) * 4, 0x5A, dtype=np.uint8)
            st, uf = pack_host(rows, 1, np.array([1], np.int32), np.array([flipped], np.uint8), 4, cols, first_col, ploidy, packed, 1, 0)
            words = packed.view(np.uint32)
            assert [(int(words[0]) >> (2 * i)) & 3 for i in range(4)] == [v if isinstance(v, int) else 0 for v in line]
            assert int(words[0]) >> 8 == 0  # padding individuals hold 0
            assert (words[1:] == 0xFFFFFFFF).all()  # padding sites: all ones
            assert st.tolist() == [4 - line.index("het") if "het" in line else 0]
            assert uf.tolist() == [4 - line.index("unfit") if "unfit" in line else 0]
    # the LOWEST individual is named: het at individuals 1 and 3 of 5 (ploidy 1); missing at 2 and 4 (flipped, ploidy 2)
    codes = np.array([[HOM_A1, HET, HOM_A2, HET, HOM_A1], [HOM_A2, HOM_A1, MISSING, HOM_A2, MISSING]], dtype=np.uint8)
    rows = (codes[:, 0] | codes[:, 1] << 2 | codes[:, 2] << 4 | codes[:, 3] << 6).astype(np.uint8)
    rows = np.stack([rows, codes[:, 4]], axis=1).ravel()  # two bytes per row
    cols, both = np.arange(5, dtype=np.int32), np.array([0, 1], np.int32)
    packed = np.zeros(tile_words(5) * 4, dtype=np.uint8)
    st, uf = pack_host(rows, 2, both, np.zeros(2, np.uint8), 5, cols, 0, 1, packed, 2, 0)
    assert st.tolist() == [5 - 1, 0] and uf.tolist() == [0, 0]
    st, uf = pack_host(rows, 2, both, np.ones(2, np.uint8), 5, cols, 0, 2, packed, 2, 0)
    assert st.tolist() == [0, 0] and uf.tolist() == [0, 5 - 2]
    assert [(int(packed.view(np.uint32)[1]) >> (2 * i)) & 3 for i in range(5)] == [2, 0, 0, 2, 0]  # the unfit fields are 0


def test_bad_indices_are_flagged_written_as_zero_and_never_read():
    rows = np.full(6, 0xFF, dtype=np.uint8)  # three rows of two bytes, 7 columns
    packed = np.full(tile_words(4) * 4, 0x11, dtype=np.uint8)
    st, uf = pack_host(rows, 2, np.array([0, 3, -1, 2], np.int32), np.zeros(4, np.uint8), 7, np.array([0, 7, 6, -2], np.int32), -1, 2,
                       packed, 4, 0)  # fmt: skip
    assert st.tolist() == [BAD_INDEX] * 4 and uf.tolist() == [0] * 4
    assert packed.view(np.uint32)[:4].tolist() == [0, 0, 0, 0] and (packed.view(np.uint32)[4:] == 0xFFFFFFFF).all()
    st, uf = pack_host(rows, 2, np.array([2, 5], np.int32), np.zeros(2, np.uint8), 7, np.arange(7, dtype=np.int32), 0, 2, packed, 4, 1)
    assert st.tolist() == [0, BAD_INDEX] and packed.view(np.uint32)[1:3].tolist() == [0, 0]


def test_argument_errors_have_the_messages_of_the_int8_decoder():
    from sai_amd import _ffi, _ffi_packed_ingest

    lib = _ffi_packed_ingest.load_host()
    rows, rib, flip = np.zeros(4, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.uint8)
    cols, packed, st, uf = np.zeros(3, np.int32), np.zeros(tile_words(3) * 4, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(**kw):
        a = dict(rows=ptr(rows), n_batch=2, row_bytes=2, n_out=1, rib=ptr(rib), flip=ptr(flip), n_cols=8, n_ind=3, cols=ptr(cols),
                 first_col=-1, ploidy=2, packed=ptr(packed), n_sites=1, out_row0=0, st=ptr(st), uf=ptr(uf), n_threads=1)  # fmt: skip
        a.update(kw)
        rc = lib.sai_bed_pack2_host(*a.values())
        return rc, lib.sai_last_error().decode()

    assert call()[0] == 0
    for kw, message in [(dict(n_cols=9), "n_cols exceeds the 4 * row_bytes genotypes of a row"), (dict(cols=None), "NULL buffer"),
                        (dict(uf=None), "NULL buffer"), (dict(first_col=6), "first_col + n_slots exceeds n_cols"),
                        (dict(ploidy=3), "ploidy must be 1 or 2"), (dict(out_row0=1), "size out of range"),
                        (dict(n_ind=0), "size out of range")]:  # fmt: skip
        rc, text = call(**kw)
        assert rc == _ffi.SAI_ERR_ARG and message in text, (kw, text)


def test_header_binding_and_library_agree_and_the_plink_header_is_untouched():
    from sai_amd import _build, _ffi, _ffi_packed_ingest, _ffi_plink

    names = abi_checks.declared_names("saihip_packed_ingest.h")
    assert names == sorted(_ffi_packed_ingest.SIGNATURES) == ["sai_bed_pack2", "sai_bed_pack2_host", "sai_packed_ingest_abi_version"]
    assert not any(n.startswith("sai_plink_") for n in names)
    lib = _ffi_packed_ingest.load()
    version = abi_checks.header_macro("saihip_packed_ingest.h", "SAI_PACKED_INGEST_ABI_VERSION")
    assert lib.sai_packed_ingest_abi_version() == _ffi_packed_ingest.SAI_PACKED_INGEST_ABI_VERSION == version == 1
    assert lib.sai_bed_pack2(None, None, 0, 0, 0, None, None, 0, 1, None, -1, 2, None, 0, 0, None, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
    # the PLINK header, its binding and the version numbers are as they were
    plink_names = abi_checks.declared_names("saihip_plink.h")
    assert plink_names == sorted(_ffi_plink.SIGNATURES) and len(plink_names) == 8
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16 and lib.sai_plink_abi_version() == _ffi_plink.SAI_PLINK_ABI_VERSION == 1
    assert "plink/bed_pack2.hip" in _build.UNITS and "plink/bed_pack2_host.cpp" in _build.HOST_UNITS
    assert ROOT / "include" / "saihip_packed_ingest.h" in _build.PUBLIC_HEADERS


def anc_file(path, chrom, positions, alleles):
    path.write_text("".join(f"{chrom}\t{p - 1}\t{p}\t{a}\n" for p, a in zip(positions, alleles)))
    return str(path)


def test_host_reader_blocks_and_errors(tmp_path):
    """``plink.load_packed`` against ``pack_numpy`` of ``plink.load_dosage``, and its two data errors: the heterozygous
    call at ploidy 1 (the int8 route's words) wins over a call that does not fit in the same row."""
    from sai_amd.utils import plink

    prefix, args = small_fileset(tmp_path)
    pops = [(["e", "a"], 2), (["d", "a", "c"], 2)]
    pos, blocks, n_matched, n_anc = plink.load_packed(prefix, "3", pops)
    assert pos.tolist() == [100, 200, 300] and (n_matched, n_anc) == (3, 0)
    for (names, ploidy), block in zip(pops, blocks):
        dos = plink.load_dosage(prefix, "3", names, [ploidy] * len(names))[1]
        assert np.array_equal(block, pack_numpy(np.where(dos < 0, 3, dos).astype(np.uint8)))
    # rows 100 and 200 flipped, 300 kept
    anc = anc_file(tmp_path / "anc.bed", "3", [100, 200, 300], ["A", "C", "A"])
    assert plink.load_dosage(prefix, "3", ["d", "e"], [2, 2], anc_allele_file=anc)[1].tolist() == [[4, 0], [0, 4], [0, 0]]
    with pytest.raises(ValueError, match=r"small.bed: missing call of sample d at variant v1 \(position 100\) in a row flipped by the "
                       r"ancestral allele: its dosage is 4, which the 2-bit layout cannot hold; read this fileset with --layout int8"):
        plink.load_packed(prefix, "3", [(["a", "b"], 2), (["c", "d", "e"], 2)], anc_allele_file=anc)
    with pytest.raises(ValueError, match="missing call of sample e at variant v2"):
        plink.load_packed(prefix, "3", [(["e"], 2)], anc_allele_file=anc, start=150)
    pos, blocks, _, _ = plink.load_packed(prefix, "3", [(["d", "e"], 1)], anc_allele_file=anc, end=250)  # ploidy 1: missing flipped is 2
    assert np.array_equal(blocks[0], pack_numpy(np.array([[2, 0], [0, 2]], dtype=np.uint8)))
    # row 100 holds a missing call of d (flipped, ploidy 2: unfit) and a heterozygous call of b (ploidy 1): the het is reported
    with pytest.raises(ValueError, match="heterozygous call of sample b at variant v1 .position 100., but the sample is configured with ploidy 1"):
        plink.load_packed(prefix, "3", [(["d", "a"], 2), (["a", "b"], 1)], anc_allele_file=anc)
    with pytest.raises(ValueError, match="SAI_AMD_INGEST_BUFFER of 1 bytes is smaller than one row"):
        plink.load_packed(prefix, "3", pops, buffer_bytes=1)


def test_memory_estimate_is_one_times_the_bed(tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod

    prefix, _ = small_fileset(tmp_path)
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "12")  # the .bed is 9 bytes: 36 resident as int8, 9 as packed2
    assert sai_mod.chunks_for_memory(prefix, layout="int8") == sai_mod.chunks_for_memory(prefix) == 3
    assert sai_mod.chunks_for_memory(prefix, layout="packed2") == sai_mod.chunks_for_memory(prefix + ".bed", layout="packed2") == 1


def test_what_packed2_refuses_before_reading(tmp_path, in_repo_root, monkeypatch):
    from sai_amd import sai as sai_mod

    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    prefix, _ = small_fileset(tmp_path)
    with open(prefix + ".bed", "r+b") as f:
        f.truncate(3)  # nothing may be read: this .bed holds its magic bytes and no genotype at all
    uq = "tests/data/example.u_and_q.config.yaml"
    dd = str(tmp_path / "with_dd.yaml")
    with open(dd, "w") as f:
        f.write(open(uq).read().replace("\nploidies:", "  DD: true\nploidies:", 1))
    ask = dict(chr_name="3", win_len=100, win_step=50, anc_allele_file=None, output_file=str(tmp_path / "o" / "s.tsv"))
    with pytest.raises(ValueError, match=r"^layout 'packed2' reads a PLINK 1 fileset \(.bed \+ .bim \+ .fam\) only, which tests/data/example.vcf is not\.$"):
        sai_mod.score(vcf_file="tests/data/example.vcf", config=uq, num_workers=1, layout="packed2", **ask)
    with pytest.raises(ValueError, match=r"^layout 'packed2' serves the U and Q statistics only, but DD is configured\.$"):
        sai_mod.score(vcf_file=prefix + ".bed", config=dd, num_workers=1, layout="packed2", **ask)
    with pytest.raises(ValueError, match=r"^layout 'packed2' runs in one process on one GPU: use num_workers=1 outside a rank job"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=2, layout="packed2", **ask)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match=r"^layout 'packed2' runs in one process on one GPU"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=1, layout="packed2", **ask)
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    monkeypatch.setenv("SAI_AMD_LAYOUT", "packed2")  # the environment's default counts like the argument
    with pytest.raises(ValueError, match=r"^layout 'packed2' is decoded on the GPU: it cannot be combined with SAI_AMD_INGEST=host\.$"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=1, **ask)
    monkeypatch.delenv("SAI_AMD_INGEST")
    with pytest.raises(ValueError, match="layout must be one of int8, packed2, not 'int4'"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=1, layout="int4", **ask)
    assert sai_mod.resolve_layout() == "packed2" and sai_mod.resolve_layout("int8") == "int8"
    monkeypatch.delenv("SAI_AMD_LAYOUT")
    assert sai_mod.resolve_layout() == "int8"
    assert not (tmp_path / "o").exists()  # refused before the output files are opened


def test_command_line_lists_the_layout():
    res = sai_cli("score", "--help")
    assert res.returncode == 0 and "--layout {int8,packed2}" in res.stdout and "SAI_AMD_LAYOUT" in res.stdout
    res = sai_cli("score", "--vcf", "tests/data/example.vcf", "--chr-name", "21", "--output", "o.tsv", "--config",
                  "tests/data/example.u_and_q.config.yaml", "--layout", "int4")  # fmt: skip
    assert res.returncode == 2 and "invalid choice: 'int4'" in res.stderr


@pytest.fixture(scope="module")
def pack2_program(tmp_path_factory):
    """tests/native/bed_pack2_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    return native_build.dump_program("bed_pack2_dump", tmp_path_factory)["san"]


def test_host_decoder_is_clean_under_asan_ubsan(tmp_path, pack2_program):
    """The host decoder run (not only compiled) under the sanitizers as a program of its own, on rows in a file: the
    same block, status and unfit as the library, for runs, gathers, cut calls and indices out of range."""
    rng = np.random.default_rng(77)
    for n_ind, n_sites, first_col, ploidy, cut in [(1, 1, 0, 2, 0), (17, 65, 3, 1, 37), (65, 130, -1, 2, 64), (130, 63, 1, 2, 37), (64, 64, -1, 1, 0)]:
        n_cols = n_ind + 9
        row_bytes = (n_cols + 3) // 4
        n_batch = n_sites + 2
        rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)
        rib = rng.permutation(n_batch)[:n_sites].astype(np.int32)
        if n_sites > 2:
            rib[1] = n_batch  # a row outside the batch
        flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
        cols = np.arange(first_col, first_col + n_ind, dtype=np.int32) if first_col >= 0 else rng.integers(-1, n_cols + 1, size=n_ind).astype(np.int32)
        (tmp_path / "rows.bin").write_bytes(rows.tobytes())
        res = native_build.run_native(pack2_program, [tmp_path / "rows.bin", row_bytes, n_cols, ploidy, first_col, cut, 3,
                                                      ",".join(map(str, rib)), ",".join(map(str, flip)), ",".join(map(str, cols))])  # fmt: skip
        assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
        lines = res.stdout.splitlines()
        fields, want_st, want_uf = expect(rows, row_bytes, rib, flip, n_cols, cols, ploidy)
        assert [int(v) for v in lines[0].split()] == want_st.tolist() and [int(v) for v in lines[1].split()] == want_uf.tolist()
        assert bytes.fromhex(lines[2]) == pack_numpy(fields).tobytes()
        packed = np.zeros(pack_numpy(fields).size, dtype=np.uint8)
        st, uf = pack_host(rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, packed, n_sites, 0)
        assert st.tolist() == want_st.tolist() and uf.tolist() == want_uf.tolist() and packed.tobytes() == bytes.fromhex(lines[2])
    res = native_build.run_native(pack2_program, [tmp_path / "rows.bin", 2, 9, 2, 0, 0, 1, 0, 0, 0])
    assert res.returncode == 3 and "n_cols exceeds the 4 * row_bytes genotypes of a row" in res.stderr and "Sanitizer" not in res.stderr
