"""The .csi index of a BCF file on the CPU: the query against brute force, the host route with and without it, every way
an index can be wrong, the knob, the header and its binding, and the stand-alone program under the sanitizers."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_checks
import bcf_builder as B
import csi_builder as X
import csi_cases as K
import native_build
from conftest import GOLDEN, ROOT

NONE, SEEK, WALK = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(autouse=True)
def index_on(monkeypatch):
    monkeypatch.delenv("SAI_AMD_BCF_INDEX", raising=False)


def open_index(path, size):
    from sai_amd import _ffi_bcf_index

    lib, handle = _ffi_bcf_index.load_host(), C.c_void_p()
    rc = lib.sai_bcf_index_open(os.fsencode(path), size, C.byref(handle))
    return lib, (handle if rc == 0 else None)


def query(lib, handle, tid, start, end):
    answer, v = C.c_int32(), C.c_uint64()
    assert lib.sai_bcf_index_query(handle, tid, -1 if start is None else start, -1 if end is None else end, C.byref(answer), C.byref(v)) == 0
    return int(answer.value), int(v.value)


def same(a, b) -> bool:
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def check_against_brute_force(lib, handle, recs, tid, grid, min_shift, depth) -> dict:
    """Every region of ``grid`` for contig ``tid``; -> how often each answer came, and how often v lay behind the
    contig's first record."""
    mine = [r for r in recs if r["chrom"] == tid]
    starts = {r["voff"] for r in mine}
    rng = 1 << (min_shift + 3 * depth)
    seen = {NONE: 0, SEEK: 0, WALK: 0, "later": 0, "exact": 0}
    for start, end in grid:
        beg, fin = 0 if start is None else start - 1, rng if end is None else min(end, rng)
        answer, v = query(lib, handle, tid, start, end)
        seen[answer] += 1
        if beg >= rng or fin <= beg:
            assert answer == WALK, (tid, start, end)
            continue
        first = next((r for r in mine if r["pos0"] >= beg), None)  # the first record with POS >= start
        overlap = any(r["pos0"] < fin and r["pos0"] + max(r["rlen"], 1) > beg for r in mine)
        assert answer in (NONE, SEEK), (tid, start, end, answer)
        if answer == NONE:
            assert not overlap, (tid, start, end)
        else:
            assert v in starts and (first is None or v <= first["voff"]), (tid, start, end, v, first)
            seen["later"] += v > mine[0]["voff"]
            seen["exact"] += first is not None and v == first["voff"]
    return seen


def test_worked_example(tmp_path):
    """tests/golden/csi_worked_example.hex: the index of the BCF worked example, field by field; the builder reproduces
    it, the reader reads it and the host route begins where it says."""
    from sai_amd.utils import bcf

    unhex = lambda name: bytes.fromhex("".join(ln.split("#")[0] for ln in (GOLDEN / name).read_text().split("\n")))  # noqa: E731
    stream, want = unhex("bcf_worked_example.hex"), unhex("csi_worked_example.hex")
    path = tmp_path / "worked.bcf"
    path.write_bytes(b"".join(B.bgzf_members(stream)))
    recs = X.records_of(path.read_bytes())
    assert [(r["voff"], r["pos0"]) for r in recs] == [(0x99, 9), (0xC8, 10), (0x100, 10), (0x12D, 39)] and recs[-1]["end"] == 0x15C
    assert X.index_stream(recs, 3, 1) == want
    X.write_index_bytes(path, want)
    lib, handle = open_index(str(path) + ".csi", path.stat().st_size)
    info = [C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()]
    assert lib.sai_bcf_index_info(handle, *[C.byref(x) for x in info]) == 0 and [x.value for x in info] == [3, 1, 1, 0]
    for (start, end), answer in {(None, None): (SEEK, 0x99), (11, 11): (SEEK, 0x99), (12, 16): (SEEK, 0x99), (17, None): (SEEK, 0x12D),
                                 (17, 32): (SEEK, 0x12D), (40, 40): (SEEK, 0x12D), (41, None): (NONE, 0), (64, 64): (NONE, 0), (65, None): (WALK, 0),
                                 (30, 20): (WALK, 0)}.items():  # fmt: skip
        assert query(lib, handle, 0, start, end) == answer, (start, end)
    assert query(lib, handle, 1, 1, 5)[0] == WALK and query(lib, handle, -1, 1, 5)[0] == WALK
    lib.sai_bcf_index_close(handle)
    # one member holds the header and every record: coffset 0 lies inside the header's members, so nothing is seeked
    trace = {}
    pos, dos, n_matched, n_anc = bcf.load_dosage(path, "5", ["c", "a"], [3, 1], 11, 40, trace=trace)
    assert pos.tolist() == [11, 11, 40] and dos.tolist() == [[3, 2], [-1, 0], [-1, 1]] and not trace["seek"]["made"]
    # the same records in members of 64 bytes: now the region's walk begins at the record 5:40
    small = tmp_path / "small.bcf"
    small.write_bytes(b"".join(B.bgzf_members(stream, member_size=64)))
    X.write_csi(small, 3, 1)
    got = bcf.load_dosage(small, "5", ["a", "b", "c"], [2, 2, 2], 20, None, trace=trace)
    assert got[0].tolist() == [40] and got[1].tolist() == [[2, 1, 0]] and got[2:] == (1, 0)
    assert trace["seek"]["made"] and trace["seek"]["voffset"] == X.records_of(small.read_bytes())[3]["voff"]
    assert trace["seek"]["file_bytes"] < small.stat().st_size


@pytest.mark.parametrize("min_shift,depth", K.LAYOUTS)
def test_the_query_against_brute_force(tmp_path, min_shift, depth):
    path = K.write_bcf(tmp_path / "a.bcf")
    recs = K.records(path)
    for pseudo, no_coor in ((True, True), (False, False), (True, False)):
        X.write_csi(path, min_shift, depth, pseudo=pseudo, n_no_coor=no_coor)
        lib, handle = open_index(path + ".csi", os.path.getsize(path))
        assert handle is not None
        n_no_coor = C.c_int64()
        assert lib.sai_bcf_index_info(handle, None, None, None, C.byref(n_no_coor)) == 0 and n_no_coor.value == (0 if no_coor else -1)
        none = 0
        for tid in (0, 1, 2):
            seen = check_against_brute_force(lib, handle, recs, tid, K.regions(recs, tid, min_shift, depth), min_shift, depth)
            assert seen[SEEK] > 50 and seen[WALK] > 0 and seen["later"] > 30 and seen["exact"] > 10, (tid, seen)
            none += seen[NONE]
        assert none > 0  # behind the last record of a contig -- unless a long record reaches there, as on contig 2
        lib.sai_bcf_index_close(handle)


def test_the_files_hold_what_they_promise(tmp_path):
    path = K.write_bcf(tmp_path / "a.bcf")
    data = open(path, "rb").read()
    recs, members = K.records(path), [m for m in X.members_of(data) if m[1]]
    assert len(members) > 30 and len(recs) == 420
    isize = {off: len(text) for off, text in members}
    header_bytes = 9 + int.from_bytes(b"".join(t for _, t in members)[5:9], "little")
    # the first record of contig 1 lies directly behind the header, in a member that holds header bytes
    assert recs[0]["chrom"] == 0 and recs[0]["g"] == header_bytes and recs[0]["voff"] & 0xFFFF > 0
    for min_shift, depth in K.LAYOUTS:
        X.index_stream(recs, min_shift, depth)  # sets r["bin"]
        mine = [r for r in recs if r["chrom"] == 1]
        levels = {max(lv for lv in range(depth + 1) if X.level_start(lv) <= r["bin"]) for r in mine}
        assert {0, 1, depth} <= levels, (min_shift, depth, levels)  # levels 0 and 1 hold the long records
        assert len({r["bin"] for r in mine if r["bin"] >= X.level_start(depth)}) > 30
        assert any(r["pos0"] >= 1 << (min_shift + 3 * depth) for r in mine) == ((min_shift, depth) != (4, 3))
        assert K.empty_leaf(recs, 1, min_shift) is not None
        # a record that the index names as the start of a chunk, spans two members and starts within 32 bytes of its member's end
        firsts = {}
        for r in mine:
            firsts.setdefault(r["bin"], r)
        assert any(r["voff"] >> 16 != r["end"] >> 16 and (r["voff"] & 0xFFFF) + 32 > isize[r["voff"] >> 16] for r in firsts.values())


def test_defaults_and_positions_up_to_half_a_billion(tmp_path):
    from sai_amd.utils import bcf

    rng = np.random.default_rng(3)
    pos = sorted(int(p) for p in np.concatenate([rng.integers(1, 5 * 10**8, 150), rng.integers(16384 * 9000, 16384 * 9003, 40), [16384, 16385, 5 * 10**8]]))
    head = ["##fileformat=VCFv4.2", "##contig=<ID=1>", "##contig=<ID=2>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb"]
    rows = [f"{c}\t{p}\t.\tA\tC\t.\t.\t.\tGT\t{k % 2}|1\t0/{k % 2}" for c in ("1", "2") for k, p in enumerate(pos)]
    path = B.write_bcf(tmp_path / "wide.bcf", "\n".join(head + rows) + "\n", member_size=900)
    X.write_csi(path)
    recs = K.records(path)
    lib, handle = open_index(path + ".csi", os.path.getsize(path))
    info = [C.c_int32(), C.c_int32(), C.c_int32()]
    assert lib.sai_bcf_index_info(handle, *[C.byref(x) for x in info], None) == 0 and [x.value for x in info] == [14, 5, 2]
    grid = K.regions(recs, 1, 14, 5)
    seen = check_against_brute_force(lib, handle, recs, 1, grid, 14, 5)
    assert seen[SEEK] > 50 and seen["later"] > 30 and seen[WALK] > 0
    lib.sai_bcf_index_close(handle)
    for start, end in grid[::7]:
        trace = {}
        got = bcf.load_dosage(path, "2", ["b", "a"], [2, 1], start, end, trace=trace)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("SAI_AMD_BCF_INDEX", "0")
            assert same(got, bcf.load_dosage(path, "2", ["b", "a"], [2, 1], start, end)), (start, end)


@pytest.mark.parametrize("min_shift,depth", K.LAYOUTS[:2])
def test_the_host_route_with_and_without_the_index(tmp_path, monkeypatch, min_shift, depth):
    """Blocks, positions and counts for the grid of regions, with and without ancestral alleles; for every contig."""
    from sai_amd.utils import bcf

    path = K.write_bcf(tmp_path / "a.bcf")
    plain = K.write_bcf(tmp_path / "plain.bcf")  # the same bytes with no index beside them
    X.write_csi(path, min_shift, depth)
    recs, anc = K.records(path), K.anc_file(tmp_path / "anc.bed", path)
    order, ploidies = list(reversed(K.SAMPLES))[:4], [2, 1, 3, 2]
    made = flipped = 0
    for chrom, tid in (("2", 1), ("1", 0), ("3", 2)):
        for start, end in K.regions(recs, tid, min_shift, depth)[:: 1 if tid == 1 else 5]:
            for a in (None, anc) if tid == 1 else (None,):
                trace = {}
                got = bcf.load_dosage(path, chrom, order, ploidies, start, end, a, trace=trace)
                want = bcf.load_dosage(plain, chrom, order, ploidies, start, end, a)
                assert same(got, want), (chrom, start, end, a)
                made += trace["seek"]["made"]
                flipped += a is not None and len(got[0]) > 0
                if chrom == "1" and start in (None, 1):  # its records begin in the header's member: read on from there
                    assert not trace["seek"]["made"]
    assert made > 100 and flipped > 20
    # the knob
    monkeypatch.setenv("SAI_AMD_BCF_INDEX", "0")
    trace = {}
    bcf.load_dosage(path, "2", order, ploidies, 3000, None, trace=trace)
    assert not trace["seek"]["made"]
    monkeypatch.delenv("SAI_AMD_BCF_INDEX")
    bcf.load_dosage(path, "2", order, ploidies, 3000, None, trace=trace)
    assert trace["seek"]["made"]
    # a whole-file read is never a seek
    bcf.load_dosage(path, "2", order, ploidies, trace=trace)
    assert not trace["seek"]["made"]


def test_a_region_in_the_last_quarter_reads_less_than_half_of_the_file(tmp_path):
    """The test that fails without the feature.  ``last_quarter`` checks, without the reader, that the region's first
    record lies behind 3/4 of the compressed bytes."""
    from sai_amd.utils import bcf

    path = K.write_bcf(tmp_path / "a.bcf")
    size = os.path.getsize(path)
    (start, end), first = K.last_quarter(path)
    with_index, without = {}, {}
    want = bcf.load_dosage(path, "2", K.SAMPLES, [2] * 5, start, end, trace=without)
    assert len(want[0]) >= 10 and want[0][0] == start and not without["seek"]["made"] and without["seek"]["file_bytes"] == size
    X.write_csi(path, 4, 3)
    got = bcf.load_dosage(path, "2", K.SAMPLES, [2] * 5, start, end, trace=with_index)
    assert same(got, want)
    seek = with_index["seek"]
    print("file", size, "bytes; read with the index", seek["file_bytes"], "in", seek["members"], "members; without", without["seek"])
    assert seek["made"] and 0 < seek["voffset"] <= first["voff"] and seek["file_bytes"] < size / 2 and seek["members"] < without["seek"]["members"] / 2


def test_every_way_an_index_can_be_wrong(tmp_path):
    from sai_amd.utils import bcf

    path, other = K.write_bcf(tmp_path / "a.bcf", level=0), K.write_bcf(tmp_path / "b.bcf", level=0, rotate_ids=1)
    size = os.path.getsize(path)
    assert os.path.getsize(other) == size
    (start, end), first = K.last_quarter(path)
    ask = dict(chr_name="2", samples=K.SAMPLES, ploidies=[2] * 5, start=start, end=end)
    plain = {}
    want = bcf.load_dosage(path, **ask, trace=plain)
    X.write_csi(path, 4, 3)
    trace = {}
    assert same(bcf.load_dosage(path, **ask, trace=trace), want) and trace["seek"]["made"]  # the control: a right index is used
    # every truncation at a field boundary is refused by the reader, but the one that only drops n_no_coor
    good = X.index_stream(K.records(path), 4, 3)
    bounds = K.field_boundaries(good)
    assert len(bounds) > 200 and bounds[-1] == len(good) and bounds[-2] == len(good) - 8
    for cut in bounds[:-1]:
        X.write_index_bytes(path, good[:cut])
        lib, handle = open_index(path + ".csi", size)
        assert (handle is not None) == (cut == len(good) - 8), cut
        if handle is not None:
            lib.sai_bcf_index_close(handle)
        else:
            assert b"the index is not used" in lib.sai_last_error()
    # what the other file's index says for the region is no record start of this file
    X.write_csi(other, 4, 3)
    lib, handle = open_index(other + ".csi", size)
    answer, v = query(lib, handle, 1, start, end)
    lib.sai_bcf_index_close(handle)
    assert answer == SEEK and v not in {r["voff"] for r in K.records(path)}
    cases = K.wrong_indexes(path, other)
    assert len(cases) == 13
    for name, write in cases:
        write()
        trace = {}
        got = bcf.load_dosage(path, **ask, trace=trace)
        assert same(got, want), name
        assert not trace["seek"]["made"] and trace["seek"]["file_bytes"] >= plain["seek"]["file_bytes"] == size, (name, trace["seek"])
    # a chain that breaks behind a right seek: the read is made again from the start and words the error of the unindexed read
    def damage(i, rec):
        K._long(i, rec)
        if i == 355:
            rec["l_shared"] = 23

    broken = B.write_bcf(tmp_path / "broken.bcf", K.vcf_text(), member_size=K.MEMBER, level=0, on_record=damage)
    assert os.path.getsize(broken) == size  # stored blocks: every offset is that of `path`
    X.write_index_bytes(broken, good)
    index = bcf._index_for(broken, 3000, None)
    assert index is not None
    with pytest.raises(ValueError, match=r"has l_shared = 23") as seeked:
        bcf._load_dosage(broken, "2", K.SAMPLES, [2] * 5, 3000, None, None, None, None, None, index)
    assert "record 356" not in str(seeked.value)  # counted from the seek
    with pytest.raises(ValueError, match=r"record 356 has l_shared = 23"):
        bcf.load_dosage(broken, "2", K.SAMPLES, [2] * 5, 3000, None)


def test_header_binding_and_library_agree_and_the_other_headers_are_untouched():
    from sai_amd import _build, _ffi, _ffi_bcf, _ffi_bcf_device, _ffi_bcf_index

    names = abi_checks.declared_names("saihip_bcf_index.h")
    assert names == sorted(_ffi_bcf_index.SIGNATURES) and len(names) == 9
    lib = _ffi_bcf_index.load()
    version = abi_checks.header_macro("saihip_bcf_index.h", "SAI_BCF_INDEX_ABI_VERSION")
    assert lib.sai_bcf_index_abi_version() == _ffi_bcf_index.SAI_BCF_INDEX_ABI_VERSION == version == 1
    for name in ("SAI_BCF_INDEX_NONE", "SAI_BCF_INDEX_SEEK", "SAI_BCF_INDEX_WALK"):
        assert abi_checks.header_macro("saihip_bcf_index.h", name) == getattr(_ffi_bcf_index, name)
    assert set(_ffi_bcf_index.HOST_SYMBOLS) == set(_ffi_bcf_index.SIGNATURES)
    assert lib.sai_bcf_index_open(None, 0, None) == _ffi.SAI_ERR_ARG and b"NULL argument" in lib.sai_last_error()
    # the other headers keep their entry points and their version numbers
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16
    assert _ffi_bcf.load().sai_bcf_abi_version() == _ffi_bcf.SAI_BCF_ABI_VERSION == 1 and len(_ffi_bcf.SIGNATURES) == 10
    assert _ffi_bcf_device.load().sai_bcf_device_abi_version() == _ffi_bcf_device.SAI_BCF_DEVICE_ABI_VERSION == 1 and len(_ffi_bcf_device.SIGNATURES) == 13
    for header, module in (("saihip_bcf.h", _ffi_bcf), ("saihip_bcf_device.h", _ffi_bcf_device)):
        assert abi_checks.declared_names(header) == sorted(module.SIGNATURES)
    assert "bcf/csi_index.cpp" in _build.HOST_UNITS and "bcf/csi_index.cpp" in _build.UNITS
    assert ROOT / "include" / "saihip_bcf_index.h" in _build.PUBLIC_HEADERS and "csrc/bcf/*.cpp" in abi_checks.package_data_patterns()


def test_packed2_still_refuses_with_its_pinned_sentence(tmp_path, in_repo_root, monkeypatch):
    from sai_amd import sai as sai_mod

    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    path = B.write_bcf(tmp_path / "calls.bcf", B.read_vcf_text(ROOT / "tests" / "data" / "example.vcf"), member_size=300)
    X.write_csi(path)
    assert os.path.exists(path + ".csi")
    ask = dict(chr_name="21", win_len=100, win_step=50, anc_allele_file=None, output_file=str(tmp_path / "o" / "s.tsv"))
    with pytest.raises(ValueError, match=rf"^layout 'packed2' reads a PLINK 1 fileset \(.bed \+ .bim \+ .fam\) only, which {re.escape(path)} is not\.$"):
        sai_mod.score(vcf_file=path, config="tests/data/example.u_and_q.config.yaml", num_workers=1, layout="packed2", **ask)


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------


@pytest.fixture(scope="module")
def dump_program(tmp_path_factory):
    """tests/native/csi_dump.cpp + the host units of libsaihip under ASan + UBSan with the runtimes linked in, as
    test_bcf_cpu.py::dump_programs builds its program."""
    return native_build.dump_program("csi_dump", tmp_path_factory)["san"]


def run_dump(exe, path, index, chrom, tid, regions, request, cap=4096, n_threads=3):
    flat = [-1 if x is None else x for reg in regions for x in reg]
    return native_build.run_native(exe, [path, index, chrom, tid, n_threads, cap, len(regions), *flat, *[f"{s}:{p}" for s, p in request]])


def test_the_stand_alone_program_under_the_sanitizers(tmp_path, dump_program):
    from sai_amd.utils import bcf

    path = K.write_bcf(tmp_path / "a.bcf", level=0)
    other = K.write_bcf(tmp_path / "b.bcf", level=0, rotate_ids=1)
    X.write_csi(path, 4, 3)
    recs = K.records(path)
    lib, handle = open_index(path + ".csi", os.path.getsize(path))
    regions = K.regions(recs, 1, 4, 3)[::9] + [K.last_quarter(path)[0]]
    request = [("s3", 2), ("s0", 1)]

    def expected(with_queries):
        lines = []
        for start, end in regions:
            if with_queries:
                lines.append("query %d %d" % query(lib, handle, 1, start, end))
            pos, dos, n_matched, n_anc = bcf.load_dosage(path, "2", ["s3", "s0"], [2, 1], start, end)
            lines += [f"{p} 0 {d[0]} {d[1]}" for p, d in zip(pos.tolist(), dos.tolist())] + [f"counts {n_matched} {n_anc}"]
        return lines

    res = run_dump(dump_program, path, path + ".csi", "2", 1, regions, request)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.split("\n")
    assert lines[0] == "index 4 3 3 0" and [ln for ln in lines[1:] if ln and not ln.startswith("seek")] == expected(True)
    seeks = [ln.split() for ln in lines if ln.startswith("seek")]
    assert len(seeks) == len(regions) and sum(s[1] == "1" for s in seeks) > len(regions) // 2 and int(seeks[-1][3]) < os.path.getsize(path) / 2
    # wrong indexes: one that fails a check, one of another file (every seek it names is looked at, none is taken blindly)
    bad = tmp_path / "bad.csi"
    bad.write_bytes(b"".join(B.bgzf_members(X.index_stream(recs, 4, 3)[:-21])))
    res = run_dump(dump_program, path, str(bad), "2", 1, regions, request)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.split("\n")
    assert lines[0] == "index refused" and [ln for ln in lines[1:] if ln and not ln.startswith("seek")] == expected(False)
    assert all(ln.split()[1] == "0" for ln in lines if ln.startswith("seek"))
    X.write_csi(other, 4, 3)
    res = run_dump(dump_program, path, other + ".csi", "2", 1, [regions[-1]], request)
    assert res.returncode == 0, res.stderr[-3000:]
    rows = [ln for ln in res.stdout.split("\n") if ln and ln.split()[0] not in ("index", "query", "seek")]
    assert rows == expected(False)[-len(rows):] and len(rows) > 10
    lib.sai_bcf_index_close(handle)
