"""The environment switches of the native library without a GPU and without loading it: csrc/nsf_knobs.h is the only reader,
its table, INTEGRATION.md §6 and the way the tests flip switches agree, the retired switches are gone, and the parses give what
each launcher's own parse gave before the table existed (a stand-alone program compiled from the header)."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nf-isam_amd", "csrc")
RETIRED = ("NFISAM_GRAD", "NFISAM_WEIGHTS", "NFISAM_HALF_W", "NFISAM_DIM_MAJOR_MIN", "NFISAM_LDS_PAD_KB", "NFISAM_PERSIST_BLOCKS")
KINDS = {"OFF", "ON", "SET", "CHAR", "WORD", "INT", "CLAMP", "REAL"}
ONCE = {"NFISAM_" + n for n in ("PERSIST", "PERSIST_PROBE", "FUSED_CLOSE", "WAIT_SECONDS", "PLAN_STREAM", "PERSIST_DIRECT",
                                "SLAB_MAX_TILES", "LONE_LEAN", "HELPERS", "PERSIST_SPLIT", "PERSIST_SPINS", "PERSIST_DROP",
                                "PERSIST_SCATTER")}


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def source_files(top):
    """every file under `top` that is not a build product (those live in directories _obj, _asm, _diag, __pycache__; libraries)"""
    out = []
    for path in sorted(glob.glob(os.path.join(top, "**", "*"), recursive=True)):
        dirs = os.path.relpath(path, top).split(os.sep)[:-1]
        if os.path.isfile(path) and not any(d.startswith("_") for d in dirs) and not path.endswith(".so"):
            out.append(path)
    return out


def knob_table():
    """variable -> (accessor, when, kind), one entry per X(...) line of NSF_KNOBS"""
    rows = re.findall(r'^\s*X\((\w+),\s*"(NFISAM_\w+)",\s*(\w+),\s*(\w+),', read(os.path.join(CSRC, "nsf_knobs.h")), re.M)
    names = [r[1] for r in rows]
    assert len(rows) >= 30 and len(set(names)) == len(names), names
    assert len({r[0] for r in rows}) == len(rows)
    return {var: (fn, when, kind) for fn, var, when, kind in rows}


def section6():
    text = read(os.path.join(ROOT, "INTEGRATION.md"))
    start = text.index("\n## 6. ")
    end = text.find("\n## ", start + 1)
    return text[start:end if end > 0 else len(text)]


def python_side_switches():
    found = set()
    for path in glob.glob(os.path.join(ROOT, "nf-isam_amd", "**", "*.py"), recursive=True):
        found.update(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(NFISAM_\w+)"', read(path)))
    return found


def test_the_header_is_the_only_reader_of_the_environment():
    files = source_files(CSRC)
    assert len(files) > 25 and os.path.join(CSRC, "nsf_knobs.h") in files
    for path in files:
        assert ("getenv(" in read(path)) == (os.path.basename(path) == "nsf_knobs.h"), path


def test_the_table_and_the_document_have_the_same_switches_one_row_each():
    table = knob_table()
    for var, (fn, when, kind) in table.items():
        assert when in ("CALL", "ONCE") and kind in KINDS, (var, when, kind)
        assert (when == "ONCE") == (var in ONCE), var                    # read times stay; NFISAM_RUN_AHEAD is read per run
    rows = [line.split("|") for line in section6().splitlines() if line.startswith("| `")]
    first = [re.findall(r"\b(?:NFISAM|BENCH)_\w+", r[1]) for r in rows]
    assert all(len(names) == 1 for names in first), [n for n in first if len(n) != 1]
    names = [n[0] for n in first]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    nfisam = {n for n in names if n.startswith("NFISAM_")}
    py = python_side_switches()
    assert py and py <= nfisam, py - nfisam
    assert nfisam - py == set(table), (sorted((nfisam - py) - set(table)), sorted(set(table) - (nfisam - py)))
    for r, n in zip(rows, names):
        if n in table:
            assert r[2].strip() == ("per call" if table[n][1] == "CALL" else "once per process"), n
        elif n in py:
            assert r[2].strip() == "per call", n
    assert any(n.startswith("BENCH_") for n in names)


def test_a_switch_that_a_test_flips_in_its_own_process_is_read_per_call():
    table = knob_table()
    flipped = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        text = read(path)
        for inside in re.findall(r"\b_Env\(([^)]*)\)", text):
            for var in re.findall(r"\b(NFISAM_\w+)\s*=", inside):
                flipped.setdefault(var, path)
        for var in re.findall(r'os\.environ\[\s*"(NFISAM_\w+)"\s*\]\s*=[^=]', text):
            flipped.setdefault(var, path)
    assert {"NFISAM_TRAIN", "NFISAM_RUN_AHEAD", "NFISAM_PAIR"} <= set(flipped), sorted(flipped)
    for var, path in sorted(flipped.items()):
        assert var in table, (var, path)
        assert table[var][1] == "CALL", "%s is read once per process, but %s sets it in its own process" % (var, path)


def test_the_retired_switches_are_gone():
    texts = {"INTEGRATION.md §6": section6()}
    for d in (CSRC, os.path.join(ROOT, "nf-isam_amd", "nfisam_hip")):
        texts.update((path, read(path)) for path in source_files(d))
    assert len(texts) > 27
    for where, text in texts.items():
        for name in RETIRED:
            assert not re.search(r"\b%s\b" % name, text), (name, where)


PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "nsf_knobs.h"
static int bad = 0;
#define CHECK(expr) do { if (!(expr)) { ++bad; printf("line %d: %s\n", __LINE__, #expr); } } while (0)
static void put(const char* var, const char* v) { if (v != nullptr) setenv(var, v, 1); else unsetenv(var); }
int main(int argc, char** argv) {
    if (argc > 1) {                                   // ONCE switches: one process per value, the value comes with the environment
        if (strcmp(argv[1], "spins") == 0) printf("%d\n", knob::persist_spins());
        if (strcmp(argv[1], "slab") == 0) printf("%d\n", knob::slab_max_tiles());
        if (strcmp(argv[1], "split") == 0) printf("%d\n", knob::persist_split());
        if (strcmp(argv[1], "stream") == 0) printf("%d\n", (int)knob::plan_stream("private"));
        if (strcmp(argv[1], "wait") == 0) printf("%g\n", knob::wait_seconds());
        return 0;
    }
    // the cases: unset, "0", "1", a valid value, an out-of-set value, garbage, empty
    const char* const cases[7] = {nullptr, "0", "1", nullptr /* per switch */, "3", "zz", ""};
    // OFF: on unless the first character is '0'
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "01";
      const bool want[7] = {true, false, true, false, true, true, true};
      for (int i = 0; i < 7; ++i) { put("NFISAM_DIM_MAJOR", v[i]); CHECK(knob::dim_major() == want[i]); } }
    // ON: off unless the first character is '1'
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "10";
      const bool want[7] = {false, false, true, true, false, false, false};
      for (int i = 0; i < 7; ++i) { put("NFISAM_SPAN", v[i]); CHECK(knob::span() == want[i]); } }
    // SET: the variable exists
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "yes";
      for (int i = 0; i < 7; ++i) { put("NFISAM_SPAN_DEBUG", v[i]); CHECK(knob::span_debug() == (v[i] != nullptr)); } }
    // CHAR: the first character, -1 when unset (NFISAM_PAIR: '0' and '1' force a kernel, NFISAM_HALF: '0' and '2')
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "1x";
      const int want[7] = {-1, '0', '1', '1', '3', 'z', 0};
      for (int i = 0; i < 7; ++i) { put("NFISAM_PAIR", v[i]); CHECK(knob::pair() == want[i]); put("NFISAM_HALF", v[i]); CHECK(knob::half() == want[i]); } }
    // WORD: the whole value
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "wide"; v[4] = "wider";
      for (int i = 0; i < 7; ++i) { put("NFISAM_TRAIN", v[i]); CHECK(knob::train("wide") == (i == 3)); CHECK(!knob::train("split")); }
      put("NFISAM_TRAIN", "split"); CHECK(knob::train("split") && !knob::train("wide"));
      put("NFISAM_WALK", "plain"); CHECK(knob::walk("plain")); put("NFISAM_WALK", "Plain"); CHECK(!knob::walk("plain")); }
    // INT: atoi, the default when unset; one validity rule per kernel family
    { const char* v[7]; memcpy(v, cases, sizeof(v)); v[3] = "8";
      const int raw[7] = {4, 0, 1, 8, 3, 0, 0}, dim_major[7] = {4, 4, 1, 8, 4, 4, 4}, tile_major[7] = {4, 4, 1, 8, 3, 4, 4};
      for (int i = 0; i < 7; ++i) {
          put("NFISAM_BIG_W", v[i]);
          CHECK(knob::big_w() == raw[i]); CHECK(knob::big_w_set() == (v[i] != nullptr));
          CHECK(knob::int_in_set(knob::big_w(), 1, 2, 4, 8, 4) == dim_major[i]);
          CHECK(knob::int_in_range(knob::big_w(), 1, 8, 4) == tile_major[i]);
      }
      put("NFISAM_BIG_W", "9"); CHECK(knob::int_in_set(knob::big_w(), 1, 2, 4, 8, 4) == 4 && knob::int_in_range(knob::big_w(), 1, 8, 4) == 4);
      const int t_raw[7] = {0, 0, 1, 8, 3, 0, 0}, t_dim[7] = {0, 0, 1, 8, 0, 0, 0}, t_tile[7] = {0, 0, 1, 8, 3, 0, 0};    // 0: by launch size
      for (int i = 0; i < 7; ++i) {
          put("NFISAM_TILES_PER_BLOCK", v[i]);
          CHECK(knob::tiles_per_block() == t_raw[i]);
          CHECK(knob::int_in_set(knob::tiles_per_block(), 1, 2, 4, 8, 0) == t_dim[i]);
          CHECK(knob::int_in_range(knob::tiles_per_block(), 1, 8, 0) == t_tile[i]);
      }
      put("NFISAM_CHAINS", nullptr); CHECK(!knob::chains_set());
      put("NFISAM_CHAINS", "0"); CHECK(knob::chains_set() && knob::chains() == 0);
      put("NFISAM_CHAINS", "-5"); CHECK(knob::chains_set() && knob::chains() == -5);     // (the launcher clamps to 1 .. 8)
      put("NFISAM_CHAINS", "2"); CHECK(knob::chains() == 2); }
    // CLAMP and REAL, as pure parses
    CHECK(knob::int_clamped(nullptr, 1, 26, 15) == 15 && knob::int_clamped("0", 1, 26, 15) == 1 && knob::int_clamped("26", 1, 26, 15) == 26);
    CHECK(knob::int_clamped("27", 1, 26, 15) == 26 && knob::int_clamped("40", 1, 26, 15) == 26 && knob::int_clamped("zz", 1, 26, 15) == 1);
    CHECK(knob::real_or(nullptr, 60.0) == 60.0 && knob::real_or("0.5", 60.0) == 0.5 && knob::real_or("zz", 60.0) == 0.0 && knob::real_or("", 60.0) == 0.0);
    // ONCE: the first call decides for the process
    put("NFISAM_PERSIST", "0"); CHECK(!knob::persist());
    put("NFISAM_PERSIST", "1"); CHECK(!knob::persist());
    put("NFISAM_PERSIST", nullptr); CHECK(!knob::persist());
    put("NFISAM_HELPERS", nullptr); CHECK(knob::helpers());
    put("NFISAM_HELPERS", "0"); CHECK(knob::helpers());
    put("NFISAM_PERSIST_DROP", "1"); CHECK(knob::persist_drop());
    put("NFISAM_PERSIST_DROP", "0"); CHECK(knob::persist_drop());
    put("NFISAM_WAIT_SECONDS", nullptr); CHECK(knob::wait_seconds() == 60.0);
    put("NFISAM_WAIT_SECONDS", "5"); CHECK(knob::wait_seconds() == 60.0);
    put("NFISAM_PERSIST_SPINS", "12"); CHECK(knob::persist_spins() == 12);
    put("NFISAM_PERSIST_SPINS", "40"); CHECK(knob::persist_spins() == 12);
    put("NFISAM_PLAN_STREAM", "private"); CHECK(knob::plan_stream("private"));
    put("NFISAM_PLAN_STREAM", "public"); CHECK(knob::plan_stream("private"));
    // ... while a CALL switch follows the environment (NFISAM_RUN_AHEAD: a test compares both settings in one process)
    put("NFISAM_RUN_AHEAD", nullptr); CHECK(knob::run_ahead());
    put("NFISAM_RUN_AHEAD", "0"); CHECK(!knob::run_ahead());
    put("NFISAM_RUN_AHEAD", "1"); CHECK(knob::run_ahead());
    printf("%d failed\n", bad);
    return bad != 0;
}
"""


@pytest.fixture(scope="module")
def knob_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs")
    src, exe = d / "knobs.cpp", d / "knobs"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)]
    # with the address and undefined-behaviour sanitizers where the machine has their runtime
    if subprocess.call(cmd[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + cmd[1:],
                       stderr=subprocess.DEVNULL) != 0 or subprocess.call([str(exe), "spins"], stdout=subprocess.DEVNULL,
                                                                          stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    return str(exe)


def run_with(exe, mode, var, value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NFISAM_")}
    if value is not None:
        env[var] = value
    return subprocess.check_output([exe, mode], env=env).decode().strip()


def test_the_parses_give_what_each_launcher_parsed_before(knob_program):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NFISAM_")}
    p = subprocess.run([knob_program], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().strip() == "0 failed", p.stdout.decode()


def test_once_switches_from_the_environment_of_a_child(knob_program):
    # NFISAM_PERSIST_SPINS: 1 .. 26 (the window-spanning kernel shifts 1u by this + 5); only values above 26 changed
    for value, want in ((None, 15), ("0", 1), ("15", 15), ("26", 26), ("27", 26), ("40", 26), ("12", 12), ("zz", 1), ("", 1)):
        assert int(run_with(knob_program, "spins", "NFISAM_PERSIST_SPINS", value)) == want, value
    for value, want in ((None, 128), ("0", 0), ("64", 64), ("-3", 0), ("zz", 0), ("", 0)):
        assert int(run_with(knob_program, "slab", "NFISAM_SLAB_MAX_TILES", value)) == want, value
    # NFISAM_PERSIST_SPLIT: unset (-1) is "by launch size"; SET, only a first character '1' divides the update
    for value, want in ((None, -1), ("0", ord("0")), ("1", ord("1")), ("", 0), ("zz", ord("z"))):
        assert int(run_with(knob_program, "split", "NFISAM_PERSIST_SPLIT", value)) == want, value
    for value, want in ((None, 0), ("private", 1), ("0", 0), ("1", 0), ("privately", 0), ("", 0)):
        assert int(run_with(knob_program, "stream", "NFISAM_PLAN_STREAM", value)) == want, value
    for value, want in ((None, 60.0), ("0", 0.0), ("1", 1.0), ("0.25", 0.25), ("zz", 0.0), ("", 0.0)):
        assert float(run_with(knob_program, "wait", "NFISAM_WAIT_SECONDS", value)) == want, value
