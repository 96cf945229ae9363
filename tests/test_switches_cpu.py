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


CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b")
DEFINED = re.compile(r"""extern\s+"C"[^;{(]*?\b(tacorl_[a-z0-9_]+)\s*\(""")


def test_kernel_sources_build_one_way():
    """The compile-time half of the same rule: no preprocessor conditional under csrc/ (a kernel source is the one kernel that
    ships, not a family of measurement builds), and no extern "C" entry point that include/tacorl_hip.h does not declare
    (tests/test_abi_cpu.py checks the other direction on the built library)."""
    from tests.test_abi_cpu import _header_symbols

    sources = [f for f in (ROOT / "tacorl_amd" / "csrc").iterdir() if f.suffix in (".hip", ".h")]
    lines, conditionals, defined = 0, [], set()
    for f in sources:
        text = f.read_text(errors="replace")
        for no, line in enumerate(text.splitlines(), 1):
            lines += 1
            if CONDITIONAL.match(line):
                conditionals.append(f"{f.name}:{no}: {line.strip()}")
        defined.update(DEFINED.findall(text))
    declared = set(_header_symbols())
    assert lines and defined and declared, "the scan found nothing: csrc/ has moved or the patterns no longer match"
    assert not conditionals, conditionals
    assert defined - declared == set(), f'defined extern "C" under csrc/ but not declared in tacorl_hip.h: {sorted(defined - declared)}'
