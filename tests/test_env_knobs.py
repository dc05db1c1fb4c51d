"""The RS_AMD_* knobs: csrc/rs_env.hpp is the only reader of the environment and its table
names every knob the library reads; include/reedsol.h documents the table's public rows.
(What the readers return, clamps included, is checked by tests/host/ring_main.cpp.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reed-solomon-cc_amd", "csrc")
KNOB = re.compile(r"RS_AMD_[A-Z0-9_]+")
REMOVED = ["FFT_WALK", "PDEC_RLOAD", "FFT_VMASK", "NET_VMASK", "FFT_RMULG", "HOST_GAP", "HOST_COPY2D", "LOW_ENC_PHASES"]
ROW = re.compile(r'^\s*\{"(RS_AMD_[A-Z0-9_]+)", (PUBLIC|MEASURE|TEST), (NUM|FLAG|TEXT|SET), '
                 r'(-?\w+), (-?\w+), (-?\w+), "([^"]+)"\},$', re.M)


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(*dirs):
    for d in dirs:
        for base, _, names in os.walk(os.path.join(ROOT, d)):
            if "__pycache__" in base or os.sep + "build" in base:
                continue
            for n in names:
                if not n.endswith((".so", ".pyc", ".o")):
                    yield os.path.join(base, n)


def _table():
    text = _read(os.path.join(CSRC, "rs_env.hpp"))
    body = text[text.index("kTable[] = {"):text.index("static_assert(sizeof(kTable)")]
    rows = ROW.findall(body)
    assert len(rows) == body.count('{"RS_AMD_'), "a table row the test cannot parse"
    return text, rows


def test_only_rs_env_reads_the_environment():
    for path in _files(os.path.join("reed-solomon-cc_amd", "csrc")):
        if os.path.basename(path) != "rs_env.hpp":
            assert "getenv" not in _read(path), path
    assert "getenv" in _read(os.path.join(CSRC, "rs_env.hpp"))


def test_removed_knobs_are_gone():
    names = ["RS_AMD_" + n for n in REMOVED]
    for path in _files(os.path.join("reed-solomon-cc_amd", "csrc"), "include", "tests", "tools",
                       os.path.join("reed-solomon-cc_amd", "reedsol_amd")):
        text = _read(path)
        for n in names:
            assert not re.search(n + r"(?![A-Z0-9_])", text), (path, n)


def test_table_names_every_knob_read():
    text, rows = _table()
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names) == 37
    used = set()
    for path in _files(os.path.join("reed-solomon-cc_amd", "csrc")):
        used |= set(KNOB.findall(_read(path)))
    assert set(names) == used
    # the Knob enum indexes the table: same names, same order
    enum = text[text.index("enum Knob {") + len("enum Knob {"):text.index("kKnobs")]
    assert [e.strip() for e in enum.split(",") if e.strip()] == [n[len("RS_AMD_"):] for n in names]


def test_rows_are_well_formed():
    _, rows = _table()
    val = {"kAuto": -1, "kMax": 2**31 - 1, "INT_MIN": -2**31}
    for name, cls, kind, d, lo, hi, doc in rows:
        d, lo, hi = (val.get(x, None) if x in val else int(x) for x in (d, lo, hi))
        if kind == "NUM":
            assert lo <= hi and (lo <= d <= hi or d == -1), name
        elif kind == "FLAG":
            assert (lo, hi) == (0, 1) and d in (0, 1), name
        else:
            assert (d, lo, hi) == (0, 0, 0), name


def test_header_documents_the_public_rows():
    _, rows = _table()
    header = _read(os.path.join(ROOT, "include", "reedsol.h"))
    start = header.index("Environment\n")
    block = header[start:header.index("*/", start)]
    assert set(KNOB.findall(block)) == {r[0] for r in rows if r[1] == "PUBLIC"}
    assert "RS_AMD_HOST_THREADS (1..64, default computed)" in block and "min(16, hardware threads)" in block
