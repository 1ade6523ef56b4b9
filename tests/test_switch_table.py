"""CPU-only checks of the library's environment switches (csrc/switches.h): one table, read once per handle, documented, and the
switches of the comparison-only paths that were removed are named nowhere any more.  Reads files only."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "sig_sdp_mmw_amd", "csrc")
# the switches retired together with the paths they selected (spelled in two pieces so that this file passes its own search)
RETIRED = ["MMW_" + n for n in (
    "GRAM_WAVES", "JACOBI_ROUNDS", "TRSM_ROWS", "GREEDY_SEQ", "GREEDY_RUNS", "SCHED", "SD_NB", "MF_CFG", "FACTOR_JACOBI_FIXED",
    "FACTOR_JACOBI_REL", "FACTOR_JACOBI_CAP", "FACTOR_MF_FLOOR", "DUAL_GRID", "LOSS_GRID", "TPW", "BLK_ROWS", "BLK_QUANT", "BLK_GROW")]


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def csrc_files():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))


def test_the_environment_is_read_in_the_switch_table_only():
    assert os.path.exists(os.path.join(CSRC, "switches.h"))
    for path in csrc_files():
        for no, line in enumerate(read(path).splitlines(), 1):
            if os.path.basename(path) != "switches.h":
                assert "getenv(" not in line, "%s:%d reads the environment outside switches.h" % (path, no)
            assert not re.search(r"static .*getenv", line), "%s:%d latches a switch for the whole process" % (path, no)


def test_every_switch_is_documented():
    names = sorted(set(re.findall(r"\bMMW_[A-Z0-9_]+\b", read(os.path.join(CSRC, "switches.h")))))
    assert len(names) >= 30, names
    doc = read(os.path.join(ROOT, "INTEGRATION.md"))
    for n in names:
        assert re.search(r"\b%s\b" % n, doc), "%s is in switches.h and not in INTEGRATION.md" % n


def test_retired_switches_are_named_nowhere():
    assert len(RETIRED) == 18
    paths = [os.path.join(ROOT, "INTEGRATION.md")]
    for top in ("sig_sdp_mmw_amd", "tools", "tests"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x != "__pycache__"]
            paths += [os.path.join(d, f) for f in files if not f.endswith((".so", ".pyc", ".npz", ".npy", ".bin"))]
    for path in paths:
        txt = read(path)
        for n in RETIRED:
            assert not re.search(r"\b%s\b" % n, txt), "%s still names %s" % (path, n)
