"""``sai score`` sub-command (mirror of sai/parsers/score_parser.py:27-130): same flags and
defaults."""

from __future__ import annotations

import argparse

from ..launcher import workers_from_env
from ..sai import score
from .argument_validation import existed_eigenstrat, existed_file, existed_fileset, existed_pfile, positive_int


def existed_input(value: str) -> str:
    """``--src-input``: a file, or ``PREFIX.bed`` / ``PREFIX.geno`` / ``PREFIX.pgen`` of a fileset whose files exist."""
    checks = {".bed": existed_fileset, ".geno": existed_eigenstrat, ".pgen": existed_pfile}
    for suffix, check in checks.items():
        if value.endswith(suffix):
            return check(value[: -len(suffix)]) + suffix
    return existed_file(value)


class SourceInput(argparse.Action):
    """``--src-input PATH``, which may be repeated: the first occurrence leaves the ``str`` (the namespace of one source
    file is what it was), a further one turns the value into the list of all paths in command-line order."""

    def __call__(self, parser, namespace, value, option_string=None):
        have = getattr(namespace, self.dest, None)
        setattr(namespace, self.dest, value if have is None else [*have, value] if isinstance(have, list) else [have, value])


def resolve_workers(args: argparse.Namespace) -> int:
    """``--num-workers``, else $SAI_AMD_GPUS, else 1 (the reference's CLI, score_parser.py:64).  The environment is
    read when `score` runs, not while the parser is built: a malformed value is `sai score`'s usage error only,
    never a traceback from `sai --help` or another sub-command."""
    if args.num_workers is None:
        try:
            args.num_workers = workers_from_env()
        except ValueError:
            args.score_parser.error("SAI_AMD_GPUS must be a positive integer")
    return args.num_workers


def resolve_input(args: argparse.Namespace) -> str:
    """Exactly one of ``--vcf``, ``--bfile``, ``--eigenstrat`` and ``--pfile``: the path ``score`` takes as its
    ``vcf_file`` (a fileset is handed over as ``PREFIX.bed`` / ``PREFIX.geno`` / ``PREFIX.pgen``).  Decided here, not by argparse's ``required=True``
    -- no flag is required alone -- but reported the same way, as a usage error with status 2."""
    given = [flag for flag in (args.vcf, args.bfile, args.eigenstrat, args.pfile) if flag is not None]
    if len(given) != 1:
        if args.pfile is not None:
            args.score_parser.error("exactly one of the arguments --vcf, --bfile, --eigenstrat and --pfile is required")
        if args.eigenstrat is None:
            args.score_parser.error("exactly one of the arguments --vcf and --bfile is required")
        args.score_parser.error("exactly one of the arguments --vcf, --bfile and --eigenstrat is required")
    if args.pfile is not None:
        return args.pfile + ".pgen"
    if args.eigenstrat is not None:
        return args.eigenstrat + ".geno"
    return args.vcf if args.bfile is None else args.bfile + ".bed"


def _run_score(args: argparse.Namespace) -> None:
    source = resolve_input(args)
    resolve_workers(args)
    score(
        vcf_file=source,
        chr_name=args.chr_name,
        win_len=args.win_len,
        win_step=args.win_step,
        anc_allele_file=args.anc_alleles,
        output_file=args.output,
        config=args.config,
        num_workers=args.num_workers,
        layout=args.layout,
        **({} if args.src_input is None else {"src_file": args.src_input}),
    )


def add_score_parser(subparsers) -> None:
    parser = subparsers.add_parser("score", help="Run the score command based on specified parameters.")
    parser.add_argument("--vcf", type=existed_file, default=None, help="Path to the VCF file containing variant data: plain, gzip or bgzip text, or a BGZF-compressed BCF 2.2 file "
                        "(told by its content; a raw, uncompressed BCF is refused; records with more than two GT values per sample, "
                        "triploid and higher, are decoded by a slower path of the GPU kernel).")
    # not a flag of the reference: the same genotypes as a PLINK 1 binary fileset, decoded on the GPU
    parser.add_argument("--bfile", type=existed_fileset, default=None, metavar="PREFIX",
                        help="Prefix of a PLINK 1 binary fileset (PREFIX.bed + PREFIX.bim + PREFIX.fam, variant-major) to "
                        "read instead of a VCF; A2 is taken as the reference allele and A1 as the alternative one. "
                        "Exactly one of --vcf and --bfile is required.")  # fmt: skip
    # ... or as an EIGENSOFT fileset: text EIGENSTRAT, PACKEDANCESTRYMAP or its transposed form, told apart by content
    parser.add_argument("--eigenstrat", type=existed_eigenstrat, default=None, metavar="PREFIX",
                        help="Prefix of an EIGENSOFT fileset (PREFIX.geno + PREFIX.snp + PREFIX.ind; text, packed or "
                        "transposed packed) to read instead of a VCF or a PLINK fileset; the first allele of the .snp is "
                        "taken as the reference allele and the second as the alternative one.")  # fmt: skip
    # ... or as a PLINK 2 fileset, what plink2 writes by default: its compressed records are expanded on the GPU
    parser.add_argument("--pfile", type=existed_pfile, default=None, metavar="PREFIX",
                        help="Prefix of a PLINK 2 binary fileset (PREFIX.pgen + PREFIX.pvar + PREFIX.psam) to read instead of "
                        "a VCF or another fileset; REF and ALT are what the .pvar names, hard calls are read.")  # fmt: skip
    parser.add_argument("--chr-name", dest="chr_name", type=str, required=True,
                        help="Chromosome name to analyze from the VCF file.")  # fmt: skip
    parser.add_argument("--win-len", dest="win_len", type=positive_int, default=50000,
                        help="Length of each genomic window in base pairs. Default: 50,000.")  # fmt: skip
    parser.add_argument("--win-step", dest="win_step", type=positive_int, default=10000,
                        help="Step size in base pairs between consecutive windows. Default: 10,000.")  # fmt: skip
    parser.add_argument("--anc-alleles", dest="anc_alleles", type=existed_file, default=None,
                        help="Path to the BED file with ancestral allele information. Without it, a site is "
                        "tested against both alleles (y and 1 - y) when the statistics are computed. Default: None.")  # fmt: skip
    parser.add_argument("--output", type=str, required=True, help="Output file path for saving results.")
    parser.add_argument("--config", type=existed_file, required=True,
                        help="Path to the YAML configuration file specifying the statistics to compute, ploidy "
                        "settings, and population group file paths.")  # fmt: skip
    # not a flag of the reference, whose CLI passes num_workers=1 (score_parser.py:64): the number of GPUs,
    # one worker process each (sai.py:42); the default, 1, is the reference's behaviour
    parser.add_argument("--num-workers", dest="num_workers", type=positive_int, default=None,
                        help="Number of GPUs to use, one worker process per GPU. Default: $SAI_AMD_GPUS, else 1.")  # fmt: skip
    # not a flag of the reference: how the genotypes lie in GPU memory
    parser.add_argument("--layout", choices=("int8", "packed2"), default=None,
                        help="Genotype layout in GPU memory: int8 (one byte per call, every input and statistic) or packed2 "
                        "(two bits per call, decoded straight from a PLINK 1 fileset given with --bfile or a PLINK 2 fileset given "
                        "with --pfile; U, Q, fd, df, Danc and Dplus, not DD; one worker; with --anc-alleles a missing call in a row "
                        "flipped by the ancestral allele does not fit two bits and asks for int8). Default: $SAI_AMD_LAYOUT, else int8.")  # fmt: skip
    # not a flag of the reference: the archaic sources in a file of their own
    parser.add_argument("--src-input", dest="src_input", type=existed_input, action=SourceInput, default=None, metavar="PATH",
                        help="Read the samples of the configuration's src list from this file instead of the main input, and score "
                        "the sites both files hold: anything --vcf takes (a plain, gzip or bgzip VCF, a BCF), or PREFIX.bed, "
                        "PREFIX.geno or PREFIX.pgen of a fileset. Requires --anc-alleles (the two inputs are reconciled through "
                        "the ancestral allele) and the int8 layout; the windows come from the main input. May be given up to 16 times, once "
                        "per source file: every src sample must then be held by exactly one of the files. Default: None.")  # fmt: skip
    parser.set_defaults(runner=_run_score, score_parser=parser)
