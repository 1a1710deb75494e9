"""api/hj_tuning.h, the one table of the library's environment switches, on the CPU: every row is documented in DESIGN.md section 4,
every row is run by a test - in tests/test_switch_matrix_gpu.py's own lists or in the file its ELSEWHERE names, which must really
hold the name: a switch added without a test fails here -, and Tuning::from_env() reads what the table says: a stand-alone C++
program over the header (g++, AddressSanitizer and UBSan, run directly) against the table as parsed from the text, for unset and
empty variables, values below and above the range, text that is no number and the rows whose default is "chosen where used"."""
import os
import re
import subprocess

import pytest

import test_switch_matrix_gpu as SM
from test_abi import ROOT

CSRC = os.path.join(ROOT, "hijiki_amd", "csrc")
HEADER = os.path.join(CSRC, "api", "hj_tuning.h")
K_UNSET = -0x7FFFFFFF
INT_MAX = 0x7FFFFFFF
LDS_PER_WORKGROUP = 160 * 1024                                          # gfx950: a workgroup may be given the CU's whole LDS


def parse_table():
    """-> (rows [(field, name, default, lo, hi)], flags [(field, name)]) from the two X-macro lists, as text"""
    text = open(HEADER).read()
    a, b, c = text.index("#define HJ_TUNING_TABLE(X)"), text.index("#define HJ_TUNING_FLAGS(X)"), text.index("#define HJ_X_FIELD")
    value = lambda s: int(eval(s, {"__builtins__": {}}, {"kUnset": K_UNSET}))      # noqa: E731  (1 << 20, 0x7FFFFFFF, -1, kUnset)
    rows = [(f, n, value(d), value(lo), value(hi)) for f, n, d, lo, hi in
            re.findall(r'X\((\w+), "(HJ_\w+)", ([^,()]+), ([^,()]+), ([^,()]+)\)', text[a:b])]
    flags = re.findall(r'X\((\w+), "(HJ_\w+)"\)', text[b:c])
    assert len(rows) == text[a:b].count('"HJ_') and len(flags) == text[b:c].count('"HJ_'), "a row of the table that the pattern does not read"
    return rows, flags


ROWS, FLAGS = parse_table()
NAMES = [r[1] for r in ROWS] + [f[1] for f in FLAGS]


def test_the_table_as_parsed():
    assert len(ROWS) >= 48 and len(FLAGS) >= 3 and len(set(NAMES)) == len(NAMES) and sorted(NAMES) == SM.table_names()
    assert len({r[0] for r in ROWS} | {f[0] for f in FLAGS}) == len(NAMES)
    for field, name, dflt, lo, hi in ROWS:
        assert lo <= hi and (dflt == K_UNSET or lo <= dflt <= hi), name
    unset = [r[1] for r in ROWS if r[2] == K_UNSET]
    assert unset == ["HJ_INNER_BURST", "HJ_REFILL_MIN", "HJ_LIGHT_GRID", "HJ_BVH_VOTE_SHADOW", "HJ_LIGHTMAP_SLICES"], unset


def test_every_switch_is_documented():
    """DESIGN.md section 4's table names every row; the device build's rows may stand behind its `HJ_LBVH_*` row"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    a = text.index("### Tuning switches")
    section = text[a:text.index("\n## ", a)]
    table = "\n".join(line for line in section.splitlines() if line.startswith("|"))
    named = set(re.findall(r"`(HJ_[A-Z0-9_]+\*?)`", table))
    missing = [n for n in NAMES if n not in named and not (n.startswith("HJ_LBVH_") and "HJ_LBVH_*" in named)]
    assert not missing, f"DESIGN.md section 4's table lacks {missing}"
    assert "tests/test_switch_matrix_gpu.py" in section and "test_switch_matrix_gpu.py" in open(HEADER).read()


def test_every_switch_is_run_by_a_test():
    """each name in exactly one of: the environments tests/test_switch_matrix_gpu.py runs, the files ELSEWHERE names"""
    own = {k for env in SM.MATRIX for k in env} | {k for frame in SM.FRAMES for k in frame[0]}
    assert own <= set(NAMES) and set(SM.ELSEWHERE) <= set(NAMES), sorted((own | set(SM.ELSEWHERE)) - set(NAMES))
    assert not own & set(SM.ELSEWHERE), f"in both lists: {sorted(own & set(SM.ELSEWHERE))}"
    neither = [n for n in NAMES if n not in own and n not in SM.ELSEWHERE]
    assert not neither, f"no test runs {neither}: add an environment to tests/test_switch_matrix_gpu.py, or the file that does to its ELSEWHERE"
    for name, path in SM.ELSEWHERE.items():
        assert path.startswith("tests/test_") and path != "tests/test_switch_matrix_gpu.py", (name, path)
        text = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"\b{name}\b", text), f"{path} does not name {name}"
        assert re.search(rf'"{name}"|{name}=', text), f"{path} names {name} but sets it nowhere"


def test_the_issue_s_environments_are_all_there():
    """the lists may grow, never shrink: these are the environments the matrix was introduced with"""
    have = [tuple(sorted(e.items())) for e in SM.MATRIX]
    for env in ({"HJ_STREAM_MIN_NODES": "0"}, {"HJ_PAIR_LEAVES": "0"}, {"HJ_PAIR_MIN_NODES": "1073741824"}, {"HJ_INNER_BURST": "1"},
                {"HJ_INNER_BURST": "16", "HJ_REFILL_MIN": "1"}, {"HJ_REFILL_MIN": "64"}, {"HJ_NODE_ORDER": "0", "HJ_COLLAPSE_PCT": "0"},
                {"HJ_NODE_ORDER": "1", "HJ_COLLAPSE_PCT": "1000"}, {"HJ_LEAF_GUARDS": "0"}, {"HJ_UPLOAD_DEVICE": "1"}, {"HJ_UPLOAD_DEVICE_MIN": "0"},
                {"HJ_UPLOAD_DEVICE": "1", "HJ_RL_DEBUG": "1"}):
        assert tuple(sorted(env.items())) in have, env
    frames = [tuple(sorted(f[0].items())) for f in SM.FRAMES]
    for env in ({"HJ_STREAM_MIN_NODES": "0"}, {"HJ_XCD_DEAL": "1", "HJ_WG_SMALL": "8"}, {"HJ_BATCH_CAP": "64"}, {"HJ_WG_SMALL": "1", "HJ_WG_SMALL_BLOCKS": "1073741824"},
                {"HJ_WG_SMALL_BLOCKS": "0"}, {"HJ_SLOTS": "2"}, {"HJ_SLOTS": "4"}, {"HJ_RECON_PRIORITY": "0"}, {"HJ_LDS_PAD_KB": "16"},
                {"HJ_TRACE_BOUNCES": "1"}, {"HJ_UPLOAD_TIMING": "1", "HJ_LIGHT_GRID_TIMING": "1"}):
        assert tuple(sorted(env.items())) in frames, env
    ranges = {name: (lo, hi) for _, name, _, lo, hi in ROWS}
    for env in SM.MATRIX + [f[0] for f in SM.FRAMES]:                   # every value inside the table's range
        for k, v in env.items():
            assert k not in ranges or ranges[k][0] <= int(v) <= ranges[k][1], (k, v)


def test_the_largest_lds_pad_still_launches():
    """HJ_LDS_PAD_KB is dynamic LDS on top of the path kernel's static WgSharedEnv (kernels/hj_stages.h): 2 x kHotNodes float4s and
    fewer than 1024 bytes of counters (16 560 bytes in the compiler's report at 512 hot nodes).  The table's upper bound and that sum
    must fit what a gfx950 workgroup may be given, or a launch at the bound fails without a word."""
    hot = int(re.search(r"#define HJ_HOT_NODES (\d+)", open(os.path.join(CSRC, "kernels", "hj_device.h")).read()).group(1))
    stages = open(os.path.join(CSRC, "kernels", "hj_stages.h")).read()
    assert "float4 nodes[2 * kHotNodes];" in stages and "struct WgSharedEnv : WgShared" in stages
    hi = {name: hi for _, name, _, _, hi in ROWS}["HJ_LDS_PAD_KB"]
    static_bound = 2 * hot * 16 + 1024
    assert hi * 1024 + static_bound <= LDS_PER_WORKGROUP, f"a pad of {hi} KB on {static_bound} static bytes exceeds {LDS_PER_WORKGROUP}"
    assert any(f[0] == {"HJ_LDS_PAD_KB": str(hi)} for f in SM.FRAMES), "no frame runs at the bound"


# ------------------------------------------------------------------------------------------------------------- from_env()

PROGRAM = r"""
#include "hj_tuning.h"
#include <cstdio>
int main() {
  const hjapi::Tuning t = hjapi::Tuning::from_env();
#define PRINT_ROW(field, name, dflt, lo, hi) std::printf("%s %d\n", name, t.field);
  HJ_TUNING_TABLE(PRINT_ROW)
#define PRINT_FLAG(field, name) std::printf("%s %d\n", name, t.field ? 1 : 0);
  HJ_TUNING_FLAGS(PRINT_FLAG)
  std::printf("pick %d %d\n", hjapi::Tuning::pick(hjapi::Tuning::kUnset, 7), hjapi::Tuning::pick(-1, 7));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tuning")
    src, exe = d / "print_tuning.cpp", d / "print_tuning"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(CSRC, "api"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def atoi(s):
    """C's atoi on text whose number fits an int: white space, a sign, digits; 0 when there are none"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def from_env(env):
    """what the table, as parsed, says from_env() returns under `env`"""
    out = {}
    for _, name, dflt, lo, hi in ROWS:
        v = env.get(name)
        out[name] = dflt if not v else min(hi, max(lo, atoi(v)))
    for _, name in FLAGS:
        out[name] = int(name in env)
    return out


def _per_row(f):
    return {name: str(f(dflt, lo, hi)) for _, name, dflt, lo, hi in ROWS}


ENVIRONMENTS = {
    "nothing set": {},
    "everything empty": {n: "" for n in NAMES},                          # a row: the default; a flag: present, so on
    "below the range": _per_row(lambda d, lo, hi: lo - 1),
    "far below": _per_row(lambda d, lo, hi: -INT_MAX),                  # (kUnset itself, given as a value: clamped like any other)
    "above the range": _per_row(lambda d, lo, hi: min(hi + 1, INT_MAX)),
    "far above": _per_row(lambda d, lo, hi: INT_MAX),
    "lowest": _per_row(lambda d, lo, hi: lo),
    "highest": dict(_per_row(lambda d, lo, hi: hi), HJ_RL_DEBUG="0"),   # (a flag set to 0 is set)
    "between": _per_row(lambda d, lo, hi: lo + (hi - lo) // 2),
    "no number": {n: "abc" for n in NAMES},                             # atoi: 0, then the range
    "a number, then text": {r[1]: "12abc" for r in ROWS},
    "blanks, a sign": {r[1]: " \t+3" for r in ROWS},
    "a sign alone": {r[1]: "-" for r in ROWS},
    "a fraction": {r[1]: "2.9" for r in ROWS},
    "one flag": {"HJ_TRACE_BOUNCES": "1"},
}


@pytest.mark.parametrize("what", list(ENVIRONMENTS))
def test_from_env_reads_what_the_table_says(program, what):
    env = ENVIRONMENTS[what]
    run = subprocess.run([program], env=dict(env), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])      # (a sanitizer report goes to stderr)
    lines = [line.split() for line in run.stdout.splitlines()]
    assert lines[-1] == ["pick", "7", "-1"]
    got = {k: int(v) for k, v in lines[:-1]}
    want = from_env(env)
    assert list(got) == NAMES and got == want, {k: (got[k], want[k]) for k in want if got.get(k) != want[k]}
    if what == "nothing set":
        assert all(got[n] == d for _, n, d, _, _ in ROWS) and sum(v == K_UNSET for v in got.values()) == 5
    if what == "no number":
        assert all(got[n] == min(hi, max(lo, 0)) for _, n, _, lo, hi in ROWS) and all(got[n] == 1 for _, n in FLAGS)
