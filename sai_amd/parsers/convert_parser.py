"""``sai convert`` sub-command: a VCF's calls written as a PLINK 1, a PLINK 2 or an EIGENSOFT fileset.  Not a command of the reference."""

from __future__ import annotations

import argparse
import json

from ..sai import convert
from .argument_validation import existed_file, positive_int

PROMISE = ("Reading the fileset at the ploidies it was written with gives the block the VCF reader gives, byte for byte, "
           "so `sai score` on it writes the same files as on the VCF.")  # fmt: skip
PGEN_NOTE = ("The .pgen rules were written from memory of the specification: the output is read back by this project's readers and equals "
             "its test writer's, and has not been opened with plink2.")  # fmt: skip
GENO_NOTE = ("The two hashes in the header record of a .geno follow EIGENSOFT's hasharr as remembered from admutils.c: they are unverified, "
             "because no EIGENSOFT program was at hand, and this project's reader ignores them. If convertf or an ADMIXTOOLS program reports "
             "a hash mismatch, put `hashcheck: NO` into its parameter file. EIGENSOFT programs want single-letter alleles; the alleles are "
             "written as the VCF spells them.")  # fmt: skip
LD_NOTE = ("Neighbouring variants in linkage disequilibrium are near copies of each other, and --ld-compress lets every row but the first of each "
           "16 be written as the list of its differences from an earlier row of its 16 (record types 2 and 3), where that is smaller: a "
           "synthetic panel of near-copied rows came out at less than half the bytes, rows drawn independently at the same bytes; the gain "
           "on a real panel is unmeasured. The fileset promises the same block. Reading it is slower, because the base row of every such "
           "record is expanded first: `sai score` from that panel, warm, took 11.0 ms against 8.8 ms. " + PGEN_NOTE)  # fmt: skip


def resolve_output(args: argparse.Namespace) -> None:
    """Exactly one of ``--out-bfile``, ``--out-pfile`` and ``--out-eigenstrat``.  The first two exclude each other in
    argparse's own words (a mutually exclusive group); the three-way rule is decided here and reported the same way, as
    a usage error with status 2, before anything is read or written."""
    error = args.convert_parser.error
    if args.ld_compress and args.out_pfile is None:
        error("--ld-compress goes with --out-pfile: only a .pgen holds records that list their differences from an earlier record")
    if args.out_eigenstrat is None:
        if args.out_bfile is None and args.out_pfile is None:
            error("one of the arguments --out-bfile --out-pfile is required, or --out-eigenstrat")
        if args.geno_format is not None:
            error("--geno-format goes with --out-eigenstrat: a PLINK fileset has one form")
        return
    for flag, value in (("--out-bfile", args.out_bfile), ("--out-pfile", args.out_pfile)):
        if value is not None:
            error(f"argument --out-eigenstrat: not allowed with argument {flag}")
    if args.append:
        error("--append does not go with --out-eigenstrat: the counts of a .geno sit in its header record, and the record length of the "
              "transposed form follows from them. Write one fileset per chromosome, or use --out-bfile.")  # fmt: skip


def _run_convert(args: argparse.Namespace) -> None:
    from ..utils.bed_writer import names_of

    resolve_output(args)
    extra = {}
    if args.out_eigenstrat is not None:
        from ..utils.geno_writer import labels_of

        extra = dict(out_eigenstrat=args.out_eigenstrat, geno_format=args.geno_format or "packed", labels=None if args.samples is None else labels_of(args.samples))
    try:
        summary = convert(
            vcf_file=args.vcf,
            chr_name=args.chr_name,
            out_prefix=args.out_bfile,
            out_pfile=args.out_pfile,
            ploidy=args.ploidy,
            haploid_samples=None if args.haploid is None else names_of(args.haploid),
            samples=None if args.samples is None else names_of(args.samples),
            start=args.start,
            end=args.end,
            append=args.append,
            skip_multiallelic=args.skip_multiallelic,
            **({"ld_compress": True} if args.ld_compress else {}),
            **extra,
        )
    except ValueError as exc:
        args.convert_parser.error(str(exc))
    print(json.dumps(summary))


def add_convert_parser(subparsers) -> None:
    parser = subparsers.add_parser(
        "convert", help="Write one chromosome of a VCF as a PLINK 1, PLINK 2 or EIGENSOFT binary fileset, encoded on the GPU.",
        description="Write the calls of one chromosome of a VCF as a PLINK 1 binary fileset (PREFIX.bed + PREFIX.bim + PREFIX.fam) "
        "with A2 = REF and A1 = ALT: no allele is swapped by its frequency; or, with --out-pfile, as a PLINK 2 fileset (PREFIX.pgen + "
        "PREFIX.pvar + PREFIX.psam), whose records are compressed on the GPU to about a third of the .bed; or, with --out-eigenstrat, as "
        "an EIGENSOFT fileset (PREFIX.geno + PREFIX.snp + PREFIX.ind), the form ADMIXTOOLS reads, whose first allele is REF. " + PROMISE
        + " The VCF is read without ancestral alleles; polarisation happens when the fileset is scored, from the .bim, .pvar or .snp "
        "alleles. " + PGEN_NOTE + " " + GENO_NOTE,
    )  # fmt: skip
    parser.add_argument("--vcf", type=existed_file, required=True, metavar="FILE", help="Path to the VCF file: plain, gzip or bgzip text.")
    parser.add_argument("--chr-name", dest="chr_name", type=str, required=True, metavar="C", help="Chromosome to write; one per call.")
    # not required=True: --out-eigenstrat stands beside the group, and resolve_output keeps argparse's sentence
    out = parser.add_mutually_exclusive_group(required=False)
    out.add_argument("--out-bfile", dest="out_bfile", type=str, default=None, metavar="PREFIX",
                     help="Prefix of the PLINK 1 fileset to write. An existing PREFIX.bed is refused without --append.")  # fmt: skip
    out.add_argument("--out-pfile", dest="out_pfile", type=str, default=None, metavar="PREFIX",
                     help="Prefix of the PLINK 2 fileset to write. An existing PREFIX.pgen is refused, and so is --append: the record table "
                     "of a .pgen sits at the front of the file. Write one fileset per chromosome, or use --out-bfile.")  # fmt: skip
    parser.add_argument("--ld-compress", dest="ld_compress", action="store_true", help="With --out-pfile only. " + LD_NOTE)
    parser.add_argument("--out-eigenstrat", dest="out_eigenstrat", type=str, default=None, metavar="PREFIX",
                        help="Prefix of the EIGENSOFT fileset to write: PREFIX.geno, PREFIX.snp (`ID CHROM 0.0 POS REF ALT`; an ID of `.` is "
                        "written CHROM:POS) and PREFIX.ind (`NAME U LABEL`; LABEL, the population to ADMIXTOOLS, is the second word of the "
                        "sample's line in the --samples file, else the name). An existing PREFIX.geno is refused, and so is --append. "
                        "Exactly one of --out-bfile, --out-pfile and --out-eigenstrat is required.")  # fmt: skip
    parser.add_argument("--geno-format", dest="geno_format", choices=("packed", "transposed"), default=None,
                        help="Form of the .geno, with --out-eigenstrat only: packed (PACKEDANCESTRYMAP, `GENO`: one record per variant) or "
                        "transposed (`TGENO`: one record per individual). Default: packed.")  # fmt: skip
    parser.add_argument("--ploidy", type=int, choices=(1, 2), default=2, help="Ploidy the samples are read at. Default: 2.")
    parser.add_argument("--haploid", type=existed_file, default=None, metavar="FILE",
                        help="File of sample names (first word of each line) that are read at ploidy 1; all others at --ploidy.")  # fmt: skip
    parser.add_argument("--samples", type=existed_file, default=None, metavar="FILE",
                        help="File of sample names (first word of each line) to write, in this order. Default: every sample of the VCF in column order.")  # fmt: skip
    parser.add_argument("--start", type=positive_int, default=None, metavar="N", help="First position to write (inclusive). Default: the chromosome's first.")
    parser.add_argument("--end", type=positive_int, default=None, metavar="N", help="Last position to write (inclusive). Default: the chromosome's last.")
    parser.add_argument("--append", action="store_true",
                        help="Add the rows to an existing fileset of the same samples: chromosome after chromosome into one fileset, or a "
                        "chromosome larger than the GPU's memory range by range. On an error the files are cut back to what they were.")  # fmt: skip
    parser.add_argument("--skip-multiallelic", dest="skip_multiallelic", action="store_true",
                        help="Drop and count the records whose ALT holds more than one allele instead of refusing the file.")  # fmt: skip
    parser.set_defaults(runner=_run_convert, convert_parser=parser)
