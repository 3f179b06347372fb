"""The library's environment switches have one place: csrc/switches.cpp reads them (read_switches()), csrc/switches.h describes them, and
the README's switch paragraph lists exactly the names of that table, in its order.  A source scan: no build, no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrays_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def _table_names():
    """The "NRAYS_..." string literals of switches.cpp, in source order."""
    return re.findall(r'"(NRAYS_[A-Z0-9_]+)"', _read("nrays_amd", "csrc", "switches.cpp"))


def _readme_names():
    """The NRAYS_* names of the README paragraph that starts with "Environment switches" (up to the next blank line), in order, without
    the constants of the C ABI and the one variable the Python package reads."""
    readme = _read("README.md")
    start = readme.index("\nEnvironment switches") + 1
    paragraph = readme[start:readme.index("\n\n", start)]
    abi_names = set(re.findall(r"^\s*(?:#define\s+)?(NRAYS_[A-Z0-9_]+)\b(?!\s*/)", _read("include", "nrays_abi.h"), re.M))  # macros and enumerators (not its comments)
    return [n for n in re.findall(r"\bNRAYS_[A-Z0-9_]+", paragraph) if n not in abi_names and n != "NRAYS_HIP_LIB"]


def test_only_switches_cpp_reads_the_environment():
    readers = sorted(name for name in os.listdir(CSRC) if "getenv(" in _read("nrays_amd", "csrc", name))
    assert readers == ["switches.cpp"]


def test_every_switch_of_the_table_is_in_the_readme():
    table = _table_names()
    assert len(table) >= 52 and len(set(table)) >= 52
    missing = [n for n in dict.fromkeys(table) if n not in _readme_names()]
    assert not missing, missing


def test_every_switch_of_the_readme_is_in_the_table():
    unknown = [n for n in _readme_names() if n not in _table_names()]
    assert not unknown, unknown


def test_the_readme_lists_each_switch_once_in_the_table_order():
    assert _readme_names() == list(dict.fromkeys(_table_names()))
