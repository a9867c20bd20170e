"""The cases of tests/tokenize_cases.py, proved without a GPU: every case keeps the buffer contract of
``sai_tokenize_gt``; the statement of the genotype rules gives what the host reader gives for the same lines written
as a VCF, and refuses where and only where the host reader refuses, with its wording; the sweep reaches every
(step, lane, byte) at which a field can start and every way the kernel learns of a start; the line-end cases end where
they claim to.  test_tokenize_device.py then runs the kernel on the same cases."""

import numpy as np
import pytest

import abi_checks
import native_build
import tokenize_cases as tc

CHROM = "1"


@pytest.fixture(scope="module")
def cases():
    return tc.all_cases()


def test_every_case_keeps_the_buffer_contract(cases):
    assert len({c.name for c in cases}) == len(cases)
    for case in cases:
        tc.check_contract(case)
    assert tc.MAX_ALLELE == abi_checks.header_macro("saihip.h", "SAI_GT_MAX_ALLELE")
    assert max(len(c.text) for c in cases) < 6 << 20


# ---- the statement against the host reader ----------------------------------------------------------------------


def position_of(i: int) -> int:
    return 10 * (i + 1)


def request(case):
    """(names, ploidies, slots): the mapped slots in order, each asked for as the sample of its column."""
    col_of = {int(s): c for c, s in enumerate(case.slot_of_col) if s >= 0}
    slots = sorted(col_of)
    return [f"c{col_of[s]}" for s in slots], [int(case.ploidy[s]) for s in slots], slots


def write_lines(case, picked, folder, stem):
    """The lines ``picked`` of a case as a VCF (GT at the line's gi inside FORMAT) and, where a line is flipped, the
    ancestral-allele file that keeps or flips each of them.  -> (vcf path, anc path or None)"""
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"c{c}" for c in range(case.n_cols)) + "\n"
    body = bytearray(head.encode())
    for i in picked:
        fmt = ":".join([f"F{k}" for k in range(int(case.gi[i]))] + ["GT"])
        body += f"{CHROM}\t{position_of(i)}\t.\tA\tT\t.\t.\t.\t{fmt}\t".encode() + case.text[case.off[i] : case.off[i] + case.len[i]] + b"\n"
    vcf = folder / f"{stem}.vcf"
    vcf.write_bytes(bytes(body))
    if not any(case.flip[i] for i in picked):
        return str(vcf), None
    anc = folder / f"{stem}.anc.bed"
    anc.write_text("".join(f"{CHROM}\t{position_of(i) - 1}\t{position_of(i)}\t{'T' if case.flip[i] else 'A'}\n" for i in picked))
    return str(vcf), str(anc)


def test_statement_equals_the_host_reader(cases, tmp_path):
    """Same rows for the accepted lines of a case in one file; every refused line alone in a file of its own is refused
    by the host reader in the words the statement names.  (Without the allele-index guard in parse_lines this fails on
    ``0|1|100001`` and ``0|99999999999``: the host reader accepts the first and wraps on the second.)"""
    from sai_amd.utils.native_vcf import load_dosage

    n_refused = 0
    for case in cases:
        names, ploidies, slots = request(case)
        if not case.host:
            with pytest.raises(ValueError, match="ploidy of sample"):
                load_dosage(write_lines(case, [0], tmp_path, case.name)[0], CHROM, names, ploidies)
            continue
        accepted = np.flatnonzero(case.status == 0).tolist()
        if accepted:
            vcf, anc = write_lines(case, accepted, tmp_path, case.name)
            for threads in (1, 3):
                pos, dos, n_matched, _ = load_dosage(vcf, CHROM, names, ploidies, None, None, anc, threads)
                assert pos.tolist() == [position_of(i) for i in accepted] and n_matched == len(accepted), case.name
                want = case.rows[accepted][:, slots]
                differ = np.flatnonzero((dos != want).any(axis=1))
                assert len(differ) == 0, (case.name, vars(case.lines[accepted[differ[0]]]), dos[differ[0]].tolist(), want[differ[0]].tolist())
        for i in np.flatnonzero(case.status != 0).tolist():
            vcf, anc = write_lines(case, [i], tmp_path, f"{case.name}_{i}")
            with pytest.raises(ValueError, match=f"{case.why[i]}.* {CHROM}:{position_of(i)}\\b|record {CHROM}:{position_of(i)} has {case.why[i]}"):
                load_dosage(vcf, CHROM, names, ploidies, None, None, anc, 1)
            n_refused += 1
    assert n_refused >= 20
    assert {w for c in cases for w in c.why if w} == {tc.UNPARSABLE, tc.TOO_FEW, tc.RANGE}


@pytest.fixture(scope="module")
def gt_dump(tmp_path_factory):
    return native_build.dump_program("vcf_gt_dump", tmp_path_factory, kinds=("san",))["san"]


def test_rules_table_through_the_host_reader_under_asan_ubsan(cases, tmp_path, gt_dump):
    """The host reader alone, as a program of its own built with the sanitizers, on the files of the rules tables: the
    accepted lines give the statement's rows, every refused line its message, and no run ends with a finding (97 /
    98) -- the eleven-digit allele index was a signed overflow."""
    ran = 0
    for case in cases:
        if case.kind != "rules" or not case.host:
            continue
        names, ploidies, slots = request(case)
        samples = [f"{n}:{p}" for n, p in zip(names, ploidies)]
        accepted = np.flatnonzero(case.status == 0).tolist()
        if accepted:
            vcf, anc = write_lines(case, accepted, tmp_path, case.name)
            res = native_build.run_native(gt_dump, [vcf, CHROM, 2, anc or "-", *samples])
            assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
            lines = res.stdout.splitlines()
            assert lines[0] == f"rows {len(accepted)} {len(slots)}"
            want = [" ".join(map(str, [position_of(i), *case.rows[i][slots].tolist()])) for i in accepted]
            assert lines[1:] == want
        for i in np.flatnonzero(case.status != 0).tolist():
            vcf, anc = write_lines(case, [i], tmp_path, f"{case.name}_{i}")
            res = native_build.run_native(gt_dump, [vcf, CHROM, 1, anc or "-", *samples])
            assert res.returncode not in (97, 98) and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
            assert res.returncode == 3 and case.why[i] in res.stderr and f"{CHROM}:{position_of(i)}" in res.stderr, (vars(case.lines[i]), res.stderr[-500:])
            ran += 1
    assert ran >= 20


# ---- what the cases reach ---------------------------------------------------------------------------------------


def test_sweep_starts_cover_every_lane_and_byte_of_three_steps(cases):
    """By arithmetic on the offsets alone: for each off % 4 and each prefix the swept field starts at every (lane, byte)
    of step 0 that lies inside the line (bytes below ``off`` in lane 0 belong to the word, not to the line), of step 1
    and of step 2, and in all four ways the kernel learns of a start.  Every field of a sweep line is a selected one,
    so the starts of all fields are counted for the classes."""
    case = next(c for c in cases if c.name == "sweep")
    assert case.n_lines == 2 * 4 * (tc.SWEEP_T + 1) and tc.SWEEP_T == 3 * 256 + 8
    assert (case.slot_of_col >= 0).all() and case.n_out > case.n_cols
    swept = {}
    classes = {}
    deepest = 0
    for i, ln in enumerate(case.lines):
        assert ln.off % 4 == ln.offmod
        starts = tc.field_starts(case, i)
        assert len(starts) == case.n_cols and ln.off + ln.swept in starts
        col = starts.index(ln.off + ln.swept)
        assert col == (min(ln.swept, 1) if ln.prefix == "junk" else (ln.swept + 1) // 2)
        step, lane, k = tc.position(ln.off, ln.off + ln.swept)
        swept.setdefault((ln.prefix, ln.offmod), set()).add((min(step, 2), lane, k))
        deepest = max(deepest, step)
        for p in starts[col : col + 2]:  # the swept field and the selected field behind it
            s = tc.position(ln.off, p)[0]
            classes.setdefault((ln.offmod, min(s, 2)), set()).add(tc.start_class(ln.off, p))
    assert deepest == 3
    every = {(lane, k) for lane in range(64) for k in range(4)}
    for prefix in ("junk", "run"):
        for mod in range(4):
            got = swept[prefix, mod]
            assert {(lane, k) for s, lane, k in got if s == 0} == {(lane, k) for lane, k in every if 4 * lane + k >= mod}
            assert {(lane, k) for s, lane, k in got if s == 1} == every and {(lane, k) for s, lane, k in got if s == 2} == every
    for mod in range(4):
        assert classes[mod, 0] == {"first", "own", "below"}  # no step before step 0 to carry from
        assert classes[mod, 1] == {"own", "below", "carry"} and classes[mod, 2] == {"own", "below", "carry"}
    # the column of the swept field grows with every step of the ``run`` lines: col_base is summed over more than two steps
    assert max((ln.swept + 1) // 2 for ln in case.lines if ln.prefix == "run") > 3 * 256 // 2


def test_line_ends_have_the_residues_they_claim(cases):
    case = next(c for c in cases if c.name == "line_ends")
    seen, lane63 = set(), 0
    for i, ln in enumerate(case.lines):
        end = ln.off + ln.len
        assert (end - (ln.off & ~3)) % 256 == ln.residue and (end - (ln.off & ~3) + 255) // 256 == ln.steps
        assert (case.text[end - 1 : end] == b"\t") == ln.trailing and case.slot_of_col[-1] >= 0
        assert len(tc.field_starts(case, i)) == case.n_cols  # the last field, empty behind a trailing tab, is the last column
        seen.add((ln.residue, ln.off % 4, ln.trailing, ln.steps))
        lane63 += ln.trailing and tc.position(ln.off, end - 1)[1:] == (63, 3)
    assert {(r, m, t, s) for r in tc.END_RESIDUES for m in range(4) for t in (False, True) for s in (2, 3)} <= seen
    assert {(r, m, t, 1) for r in (0, 255) for m in range(4) for t in (False, True)} <= seen
    assert lane63 >= 8
    for n_cols, flagged in ((1, 0), (2, 1)):
        empty = next(c for c in cases if c.name == f"empty_{n_cols}col")
        assert empty.len.tolist() == [0] * 4 and sorted(empty.off % 4) == [0, 1, 2, 3] and empty.status.tolist() == [flagged] * 4
        assert flagged or (empty.rows == np.where(empty.flip[:, None] == 1, 4, -2)).all()  # one missing diploid call


def test_straddle_and_launch_cases_are_where_they_claim(cases):
    case = next(c for c in cases if c.name == "straddle")
    at = set()
    for ln in case.lines:
        step, lane, k = tc.position(ln.off, ln.off + ln.swept + ln.at)
        assert (lane, k) == (0, 0) and step * 256 == ln.boundary  # byte ``at`` of the field is the first byte of a step
        assert case.text[ln.off + ln.swept : ln.off + ln.swept + len(tc.STRADDLE)] == tc.STRADDLE
        at.add((ln.boundary, ln.off % 4, ln.at, ln.gi))
    assert len(at) == 2 * 4 * (len(tc.STRADDLE) + 1) * 2
    launch = [c for c in cases if c.kind == "launch"]
    assert sorted({(c.n_lines, c.meta.slack_bytes) for c in launch}) == [(n, s) for n in tc.LAUNCH_LINES for s in range(4)]
    for c in launch:
        assert (c.off[1:] == (c.off + c.len)[:-1]).all() and len(c.text) - int(c.off[-1] + c.len[-1]) == c.meta.slack_bytes
        assert len({row.tobytes() for row in c.rows}) == c.n_lines  # no two lines of a launch give the same row
    assert {int(c.off[-1]) % 4 for c in launch} == {0, 1, 2, 3}


def test_geometry_lines_are_accepted_and_refused_lines_have_a_twin(cases):
    for case in cases:
        if case.kind != "rules":
            assert not case.status.any(), case.name
    tables = [c for c in cases if c.name.startswith("rules")]
    assert len(tables) == 3
    for case in tables:
        for i in np.flatnonzero(case.status).tolist():
            assert (case.status[max(0, i - 3) : i] == 0).any(), (case.name, case.lines[i].note)  # an accepted line just before it
    notes = {ln.note: int(s) for c in tables for ln, s in zip(c.lines, c.status)}
    assert notes["d = 127 is kept"] == 0 and notes["d = 128 is refused"] == 1
    assert notes["the largest allele index, beyond the ploidy"] == 0 and notes["one more is refused, counted or not"] == 1
    assert notes["ploidy 63, all missing: d = -63, fd = 126"] == 0 and notes["ploidy 64, all missing: fd = 128"] == 1
    assert notes["ploidy 128, all missing: d = -128 but fd = 256"] == 1 and notes["ploidy 129, all missing: d = -129"] == 1
    assert notes["the same in the column that is not selected"] == 0 and notes["more fields than columns: the extra ones are never read"] == 0
    assert tc.gt_field(b"0x", 0, 2) == (-1, 3) and tc.gt_field(b"0|x", 0, 2) is None and tc.gt_field(b"10|2:7", 0, 2) == (12, 10)
