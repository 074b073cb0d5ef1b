"""The option keys of spfm_set_option / spfm_get_option: the engine's table
(sparsepoly_amd/csrc/spfm_options.inc.h) and the table in include/spfm.h list the same keys, once
each, and every key the repository's own Python passes to set_option / get_option is one of
them.  Text only: nothing is compiled, no device is needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one row of the engine's table: {"key", CLASS, access(...), mask, "description"},
_ROW = re.compile(r'^\s*\{"([a-z0-9_]+)",\s*(TUNING|DIAGNOSTIC|TEST_HOOK|READOUT),\s*(.*),\s*'
                  r'([A-Z0-9 |]+),\s*"[^"]*"\},?\s*$', re.M)
# one row of the header's table:  *   "key"   | values (default) | affects | when
_HEADER_ROW = re.compile(r'^ \*   "([a-z0-9_]+)"\s*\|', re.M)
_LITERAL_USE = re.compile(r'\b[sg]et_option\(\s*["\']([A-Za-z0-9_]+)["\']')


def engine_rows():
    """[(key, class, access expression, mask expression)] in table order."""
    text = open(os.path.join(ROOT, "sparsepoly_amd", "csrc", "spfm_options.inc.h")).read()
    table = text[text.index("const OptRow kOptions[] = {"):]
    table = table[:table.index("\n};")]
    rows = [m.groups() for m in _ROW.finditer(table)]
    # every line of the table that opens a row was understood
    assert len(rows) == len(re.findall(r'^\s*\{"', table, flags=re.M))
    return rows


def header_keys():
    text = open(os.path.join(ROOT, "include", "spfm.h")).read()
    start = text.index("/* -- options ---")
    section = text[start:text.index("int spfm_set_option(", start)]
    return _HEADER_ROW.findall(section)


def test_engine_table_and_header_table_list_the_same_keys_once():
    eng = [r[0] for r in engine_rows()]
    hdr = header_keys()
    assert len(eng) > 50
    assert sorted(k for k in set(eng) if eng.count(k) > 1) == []
    assert sorted(k for k in set(hdr) if hdr.count(k) > 1) == []
    assert sorted(set(eng) - set(hdr)) == [] and sorted(set(hdr) - set(eng)) == []


def test_header_has_one_option_section_without_round_wording():
    text = open(os.path.join(ROOT, "include", "spfm.h")).read()
    assert text.count("/* -- options ---") == 1
    assert not re.search(r"\bRound \d", text)


def _python_sources():
    for top in ("sparsepoly_amd", "tools", "tests"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py"):
                    yield os.path.join(dirpath, f)
    yield os.path.join(ROOT, "bench.py")


def test_every_key_the_python_code_uses_is_in_the_table():
    known = {r[0] for r in engine_rows()}
    # keys that tests pass on purpose to see the unknown-key error
    deliberate = {"no_such_option"}
    used = {}
    for path in _python_sources():
        for key in _LITERAL_USE.findall(open(path).read()):
            used.setdefault(key, os.path.relpath(path, ROOT))
    assert len(used) > 30
    unknown = {k: p for k, p in used.items() if k not in known and k not in deliberate}
    assert unknown == {}
