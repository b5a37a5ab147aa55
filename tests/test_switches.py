"""No orphan compile-time switches: every -D a build or tool passes is read by the sources, and
every DDRL_* macro the sources test is defined there or passed by a committed build or tool.
A text search for macro names, nothing more."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSERS = ["ddrl_amd/build.py", "tools/ablate.py", "tools/ablate_gnn.py", "tools/build_diag.py",
           "tools/diag_stamps.py", "tools/diag_gnn_stamps.py"]
# tested by the sources, set by hand only: the stamped thread of a per-wave -DDDRL_STAMPS build
ALLOWED = {"DDRL_STAMP_TID"}


def _read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def _passed():
    names = set()
    for rel in PASSERS:
        text = _read(rel)
        names.update(re.findall(r"-D(DDRL_\w+)", text))
        for variants in re.findall(r"^VARIANTS = \[(.*?)\]", text, re.S | re.M):   # the ablation lists: bare names
            names.update(re.findall(r"DDRL_\w+", variants))
    return names


def _sources():
    return {p: open(p).read() for d in ("ddrl_amd/csrc", "include") for p in glob.glob(os.path.join(ROOT, d, "*"))
            if os.path.isfile(p)}


def test_no_orphan_switches():
    passed, src = _passed(), _sources()
    csrc = "\n".join(t for p, t in src.items() if os.sep + "csrc" + os.sep in p)
    assert {"DDRL_BOUNDS", "DDRL_XCHG_ATOMIC", "DDRL_STAMPS", "DDRL_GNN_STAMPS", "DDRL_ABL_NO_DW2"} <= passed
    unread = sorted(n for n in passed if not re.search(rf"\b{n}\b", csrc))
    assert not unread, f"passed as -D but read by no file under ddrl_amd/csrc: {unread}"
    tested = set()
    for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", csrc, re.M):
        tested.update(re.findall(r"DDRL_\w+", line.split("//")[0]))
    defined = set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DDRL_\w+)", "\n".join(src.values()), re.M))
    orphan = sorted(tested - defined - passed - ALLOWED)
    assert not orphan, f"tested by the sources, but never defined and passed by no build or tool: {orphan}"
