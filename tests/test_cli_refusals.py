"""What `yak-amd` refuses of a command's table before it loads it -- a file that is no .yak file, a k the command does not serve, a -c outside
[1, 1023] -- with the exit code and the one line on stderr, and the usage text of the bare program.  All of it returns before any device call.  The
texts are literals here: they are what the commands have said since each was written."""
import os
import subprocess

import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")

ODD_GRAPH = "the graph is defined for an odd k only"
# command: the arguments behind the table, why it refuses an even k (None: it does not), why it refuses k >= 32, whether -c is a count in [1, 1023]
COMMANDS = {
    "depth": (["x.fa"], None, "the per-position lookup serves k below 32 only", False),
    "cover": (["x.fa"], None, "the per-position lookup serves k below 32 only", False),
    "unitigs": ([], ODD_GRAPH, "k must be below 32", True),
    "paths": (["x.fa"], ODD_GRAPH, "k must be below 32", True),
    "bubbles": ([], ODD_GRAPH, "k must be below 32", True),
    "clean": (["x.yak"], ODD_GRAPH, "k must be below 32", True),
    "correct": (["x.fq"], None, "the per-position lookup serves k below 32 only", True),
    "hetmers": ([], "a k-mer of even length has no middle base", "k must be below 32", True),
    "print": ([], None, "a k-mer can be rebuilt from its hash for k below 32 only", False),
}

USAGE = """yak-amd: driver of libyak_amd.so (lh3/yak's C API on MI355X)
    yak-amd count    count k-mers on the GPU, write a .yak table
    yak-amd qv       look the k-mers of sequences up in a .yak table
    yak-amd triobin  bin reads by the k-mers of the two parents' .yak tables
    yak-amd trioeval evaluate the phasing of an assembly by the k-mers of the two parents' .yak tables
    yak-amd inspect  the k-mer histogram of a .yak table, or the joint spectrum of two
    yak-amd chkerr   report the streaks of low k-mers of sequences against a .yak table
    yak-amd sexchr   count the sex-chromosome k-mers of two haplotype assemblies
    yak-amd print    list the k-mers of a .yak table as text
    yak-amd cntasm   count in how many assemblies each k-mer occurs, write a .yak table
    yak-amd recount  count the k-mers of a .yak table in other sequences
    yak-amd subtract the k-mers of a .yak table that are absent from a second one
    yak-amd isec     the k-mers of a .yak table that are present in every further one
    yak-amd version  print the version
  beyond the reference:
      yak-amd sum      add the counts of two or more .yak tables together
      yak-amd depth    the depth of the k-mers of each sequence, or window, in a .yak table
      yak-amd hetmers  the pairs of k-mers of a .yak table that differ in the middle base, by their two counts
      yak-amd cover    the bases of each sequence that lie inside k-mers a .yak table holds, lacks or holds too often
      yak-amd unitigs  the unitigs of the de Bruijn graph that the k-mers of a .yak table span
      yak-amd paths    sequences as paths through the unitigs of that graph (GAF)
      yak-amd bubbles  the simple bubbles of that graph: forks whose two arms join again, with their alleles
      yak-amd clean    that graph with its tips clipped and its bubbles popped, as a .yak table of the k-mers that stay
      yak-amd correct  reads with their single substitution errors repaired against a .yak table
"""


def refused(cmd, opts, table, code, line):
    r = subprocess.run([CLI, cmd] + opts + [table] + COMMANDS[cmd][0], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    lines = r.stderr.decode().splitlines(keepends=True)
    assert (r.returncode, lines[-1:], r.stdout) == (code, ["yak-amd %s: %s\n" % (cmd, line)], b""), (cmd, opts, table)
    assert all(ln.startswith("[E::yak_amd] yak header: ") for ln in lines[:-1]), lines        # the library on a file it cannot read, nothing else


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
def test_a_command_refuses_its_table(cmd, tmp_path):
    rest, even_why, why_32, has_c = COMMANDS[cmd]
    missing, short = str(tmp_path / "none.yak"), str(tmp_path / "short.yak")
    open(short, "wb").write(b"YAK\2" + b"\0" * 11)                                # 15 bytes: no whole header
    k32, k41, k21 = (os.path.join(GOLDEN, n) for n in ("nb_k32.yak", "nb_k41.yak", "nb_k21.yak"))
    for fn in (missing, short):
        refused(cmd, [], fn, 2, "%s is not a readable .yak file" % fn)
    refused(cmd, [], k32, 2, "%s has k = 32: %s" % (k32, even_why or why_32))      # an even k, where that matters, is refused before a large one
    refused(cmd, [], k41, 2, "%s has k = 41: %s" % (k41, why_32))
    if has_c:
        for c in ("0", "1024"):
            refused(cmd, ["-c", c], k21, 1, "-c must be in [1, 1023]")
            refused(cmd, ["-c" + c], k41, 2, "%s has k = 41: %s" % (k41, why_32))  # the header is looked at first


def test_correct_holds_e_to_the_tables_k():
    k21 = os.path.join(GOLDEN, "nb_k21.yak")
    for e in ("0", "22"):
        refused("correct", ["-e", e], k21, 1, "-e must be in [1, 21], the table's k")
    refused("correct", ["-e", "22", "-c", "0"], k21, 1, "-c must be in [1, 1023]")


def test_the_bare_program_prints_its_commands():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert (r.returncode, r.stderr.decode(), r.stdout) == (1, USAGE, b"")
    r = subprocess.run([CLI, "nosuch"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert (r.returncode, r.stderr.decode()) == (1, USAGE)
