"""The environment switches the package reads and the table in INTEGRATION.md name the same variables: an undocumented
switch cannot come back unnoticed, and a documented one cannot silently stop existing.  Text only: no GPU, no library."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAME = re.compile(r"TACORL_[A-Z0-9_]+")
# Every quoted "TACORL_..." literal counts as a read: that covers os.environ.get( / os.environ[ / getenv( and also a name
# handed to a wrapper or a macro around them.  (Error codes and dtype constants of the C ABI never appear quoted.)
READ = re.compile(r"""["'](TACORL_[A-Z0-9_]+)["']""")
# Rows the table may carry although nothing under tacorl_amd/ reads them: bench.py's and the tests' own settings.
BENCH_OR_TESTS_ONLY = {"TACORL_DIST_BACKEND"}
BENCH_PREFIX = "TACORL_BENCH_"


def read_in_package():
    files = list((ROOT / "tacorl_amd").rglob("*.py")) + [f for f in (ROOT / "tacorl_amd" / "csrc").iterdir() if f.is_file()]
    names = set()
    for f in files:
        names.update(READ.findall(f.read_text(errors="replace")))
    return names


def documented():
    names, in_table = set(), False
    for line in (ROOT / "INTEGRATION.md").read_text().splitlines():
        if line.startswith("| variable |"):
            in_table = True
        elif in_table and not line.startswith("|"):
            break
        elif in_table:
            names.update(NAME.findall(line.split("|")[1]))
    return names


def test_switches_read_equal_switches_documented():
    read, table = read_in_package(), documented()
    assert read and table, "the scan found nothing: the patterns no longer match the source or the table"
    outside = {n for n in table if n in BENCH_OR_TESTS_ONLY or n.startswith(BENCH_PREFIX)}
    assert not outside & read, f"listed as read by bench.py / tests only, but the package reads them: {sorted(outside & read)}"
    assert read - table == set(), f"read under tacorl_amd/ but missing from INTEGRATION.md's table: {sorted(read - table)}"
    assert table - outside - read == set(), f"in INTEGRATION.md's table but read nowhere under tacorl_amd/: {sorted(table - outside - read)}"
