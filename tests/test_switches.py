"""The environment switches and the tool citations, pinned to the tree (CPU
only; both tests read files and nothing else).

* Every ``LZ4M_*`` name the product reads from the environment has a row in
  INTEGRATION.md's "Environment switches" table, and the table has no other.
* Every ``tools/...`` path the documents and sources cite exists, unless the
  text marks it "(removed; last in ...)".
"""
import glob
import os
import re
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "python-lz4_amd")
REMOVED = r"`?\s*\(removed; last in "
HISTORICAL = {"VERDICT.md", "ADVICE.md", "SURVEY.md"}   # records of their round, left as written


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _switches_read():
    names = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        if os.path.isfile(path):
            names |= set(re.findall(r'getenv\(\s*"(LZ4M_[A-Z0-9_]+)"', _read(path)))
    for path in glob.glob(os.path.join(PKG, "lz4", "**", "*.py"), recursive=True):
        names |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(LZ4M_[A-Z0-9_]+)"', _read(path)))
    return names


def _switches_documented():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = re.search(r"^## [^\n]*Environment switches\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert section, "INTEGRATION.md has no 'Environment switches' section"
    return set(re.findall(r"^\| `(LZ4M_[A-Z0-9_]+)` \|", section.group(1), re.M))


def test_switch_list():
    read, documented = _switches_read(), _switches_documented()
    assert read, "no switch found in the sources: the patterns no longer match the code"
    assert read == documented, (f"read but not in INTEGRATION.md's table: {sorted(read - documented)}; "
                                f"in the table but not read: {sorted(documented - read)}")


def _citing_files():
    tracked = subprocess.run(["git", "ls-files", "*.md"], cwd=ROOT, capture_output=True, text=True)
    if tracked.returncode == 0 and tracked.stdout.strip():
        docs = [f for f in tracked.stdout.split() if "/" not in f]
    else:   # an exported tree without its .git
        docs = [os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "*.md"))]
    files = [os.path.join(ROOT, f) for f in docs if f not in HISTORICAL]
    files += [os.path.join(ROOT, "include", "lz4m.h"), os.path.join(ROOT, "bench.py")]
    files += [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.isfile(p)]
    return files


def test_tool_citations():
    missing = []
    for path in _citing_files():
        text = _read(path)
        for m in re.finditer(r"tools/[A-Za-z0-9_./*-]+", text):
            cited = m.group(0).rstrip(".")   # (a sentence's full stop; a name may hold a shell pattern)
            if re.match(REMOVED, text[m.end():]):
                continue
            if not glob.glob(os.path.join(ROOT, cited)):
                missing.append(f"{os.path.relpath(path, ROOT)}: {cited}")
    assert not missing, "cited tools that do not exist (mark them '(removed; last in <commit>)'): " + "; ".join(missing)
