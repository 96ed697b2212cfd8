"""The pointer contract of the core entry points (include/pss.h, "Pointer alignment"), held together without a GPU:

- every exported function that takes a device pointer is either a row of tests/view_cases.py (run on views of buffers by
  tests/test_gpu_views_of_buffers.py) or named in view_cases.ALREADY_OFFSET / OPAQUE_BYTES with the suite that offsets its pointers: a new
  export cannot skip the question;
- every row's entry point refuses pointers below their record in its launch code: a PSS_ALIGNED line with the entry point's name and a
  PSS_P(argument, bytes) for every device pointer of the prototype whose record is wider than a byte, with the record the header's table
  gives its type — the text of the refusal ("<entry>: <argument> must be <n>-byte aligned") is built from exactly those;
- the header states the contract once, PARITY.md holds the decision table with the file and line of every wide access, and each access it
  lists still stands in the function it names.
"""
import os
import re

import view_cases as VC
from pyspecsdr_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyspecsdr_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def prototypes():
    """name -> [(type, parameter name)] of every function include/pss.h declares."""
    text = re.sub(r"/\*.*?\*/", " ", _read("include", "pss.h"), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|long|void|uint32_t|float|const char \*|void \*)\s*(pss_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            pm = re.match(r"(.*?)(\w+)$", p)
            if pm:
                params.append((pm.group(1).strip(), pm.group(2)))
        out[m.group(1)] = params
    return out


def record_of(ctype, name):
    """The header's table: bytes a device pointer of this type and name must be aligned to."""
    t = ctype.replace("const", "").replace(" ", "")
    if t == "float*":
        return 8 if name in ("d_iq", "d_out_iq") else 4
    return {"double*": 8, "int16_t*": 4, "int32_t*": 4, "uint32_t*": 4, "int8_t*": 1, "uint8_t*": 1}[t]


def device_entries():
    return {name: [(t, p) for t, p in params if p.startswith("d_") and t.endswith("*")] for name, params in prototypes().items()
            if any(p.startswith("d_") and t.endswith("*") for t, p in params)}


def test_every_export_with_a_device_pointer_is_a_row_or_has_a_suite_that_offsets_it():
    dev = device_entries()
    assert set(dev) <= set(L._SIGS), f"declared in pss.h, missing from _lib._SIGS: {sorted(set(dev) - set(L._SIGS))}"
    undeclared = [n for n in L._SIGS if n not in prototypes()]
    assert not undeclared, f"in _lib._SIGS, not declared in pss.h: {undeclared}"
    assert len(dev) >= 95, f"only {len(dev)} device entry points were parsed from pss.h"
    rows, named = set(VC.ENTRIES), set(VC.ALREADY_OFFSET) | set(VC.OPAQUE_BYTES)
    assert not rows & named, f"both a row and on a list: {sorted(rows & named)}"
    unasked = sorted(set(dev) - rows - named)
    assert not unasked, f"device entry points that are neither a row of view_cases nor listed with the suite that offsets their pointers: {unasked}"
    stale = sorted((rows | named) - set(dev))
    assert not stale, f"rows or list entries that pss.h does not declare with a device pointer: {stale}"
    for entry, suite in {**VC.ALREADY_OFFSET, **VC.OPAQUE_BYTES}.items():
        path = os.path.join(ROOT, "tests", suite)
        assert os.path.exists(path), f"{entry}: {suite} does not exist"
        method = entry[4:]
        assert re.search(r"\b" + method + r"\(|" + entry, _read("tests", suite)), f"{suite} never calls {entry}"


def _aligned_statements():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp")):
            for m in re.finditer(r'PSS_ALIGNED\(\s*[\w>-]+,\s*"(pss_\w+)"\s*,(.*?)\);', _read("pyspecsdr_amd", "csrc", name), flags=re.S):
                assert m.group(1) not in found, f"{m.group(1)} has two PSS_ALIGNED lines"
                found[m.group(1)] = (name, dict((a, int(b)) for a, b in re.findall(r"PSS_P\((\w+),\s*(\d+)\)", m.group(2))))
    return found


def test_every_row_refuses_pointers_below_their_record_in_its_launch_code():
    dev, stated = device_entries(), _aligned_statements()
    api = _read("pyspecsdr_amd", "csrc", "pss_api.cpp")
    assert 'std::string(entry) + ": " + a.name + " must be " + std::to_string(a.align) + "-byte aligned"' in api, "the refusal's text changed"
    assert "return pss_fail(ctx, PSS_E_ARG," in api[api.index("int pss_ptrs_aligned"):api.index("int pss_hip_check")]
    for entry in VC.ENTRIES:
        wide = {p: record_of(t, p) for t, p in dev[entry] if record_of(t, p) > 1}
        if not wide:
            assert entry not in stated or not stated[entry][1], f"{entry} has byte buffers only"
            continue
        assert entry in stated, f"{entry}: no PSS_ALIGNED line in the launch code"
        src, args = stated[entry]
        assert args == wide, f"{entry} ({src}): PSS_ALIGNED checks {args}, the prototype and the header's table give {wide}"


def test_the_rows_use_the_prototypes_names_and_records():
    """Where a row's argument carries a prototype's name, its layout's record is the one the launch code checks (the rows rename only
    byte buffers: d_line_a / d_line_b for the display lines)."""
    dev = device_entries()
    for r in VC.ROWS:
        proto = {p: record_of(t, p) for t, p in dev[r.entry]}
        case = r.make()
        assert case.decisions()[1] == 0, f"{r.id}: a refused argument needs its message in the source and a line in pss.h"
        for a in case.args:
            if a.name in proto:
                assert a.record == proto[a.name], f"{r.id}: {a.name} is a {a.layout} buffer (record {a.record}), the header's table gives {proto[a.name]}"
            else:
                assert a.record == 1 or r.entry.startswith("pss_ring_"), f"{r.id}: {a.name} is not a parameter of {r.entry}"


def test_the_header_states_the_contract_once():
    h = _read("include", "pss.h")
    i = h.index("/* ---- batched device entry points")
    block = h[i:h.index("int pss_spectrum_db(", i)]
    for phrase in ("Pointer alignment.", "ONE RECORD", "one sample            8 bytes", "one [L, R] pair       4", "SERVES", "BELOW its record's alignment",
                   "PSS_E_ARG", "must be <n>-byte aligned", "outputs untouched", "never writes its inputs", "no atomic operation is ever made", "PARITY.md"):
        assert phrase in block, f"include/pss.h, batched device entry points: the contract no longer says {phrase!r}"
    assert h.count("Pointer alignment.") == 1


def wide_access_table():
    """The rows of PARITY.md's decision table: (file, line at the commit that wrote the table, function, text of the access)."""
    parity = _read("PARITY.md")
    sec = parity[parity.index("## Views of buffers"):]
    return re.findall(r"^\| `(pss_[\w.]+):(\d+)` \| `([^`]+)` \| `([^`]+)` \|", sec, flags=re.M)


def test_the_decision_table_names_accesses_that_are_in_the_functions_it_names():
    """Pinned by content, as launch_caps.py pins launch lines: the access stands in the named file inside the named function (before the next
    kernel begins).  The line numbers are the reader's and may drift."""
    table = wide_access_table()
    assert len(table) >= 14, f"PARITY.md, Views of buffers: {len(table)} wide accesses listed"
    for name, _line, func, text in table:
        src = _read("pyspecsdr_amd", "csrc", name)
        assert src.count(func) == 1, f"PARITY.md names {func!r} in {name}: found {src.count(func)} times"
        body = src[src.index(func):]
        nxt = re.search(r"\n__global__ ", body[len(func):])
        body = body[:len(func) + nxt.start()] if nxt else body
        assert text in body, f"PARITY.md: `{text}` is no longer in {func.strip('( ')} of {name}"
    parity = _read("PARITY.md")
    for entry in VC.ENTRIES:
        assert f"`{entry}`" in parity[parity.index("## Views of buffers"):], f"PARITY.md, Views of buffers: {entry} is not in the table of decisions"
    assert parity.count("`pss_spectrum_db_c128`,") == 1, "an entry point is listed twice"
