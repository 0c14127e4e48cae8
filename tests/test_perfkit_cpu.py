"""CPU suite: the measuring convention of the sixteen tools/*_perf.py lives ONCE, in tools/perfkit.py, and
tools/ab.py, the one A/B driver through bench.py, stops at the first run that fails.  No GPU and no timing: perfkit.one is replaced
by a scripted clock (1.0, 2.0, 3.0, ... ms) that logs what it was given, and bench.py by a stand-in in tmp_path."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import perfkit   # noqa: E402

COMMON = {"--reps": 20, "--warmup": 3, "--only": None}
SPREAD = {**COMMON, "--spread-repeats": 5, "--out": None}
ROUNDS = {"--rounds": 6, "--reps": 5, "--warmup": 2, "--only": None, "--out": None}
# option -> default of every tool, as at the commit before the tools moved onto perfkit
OPTIONS = {
    "segmented": COMMON,
    "topk": {**COMMON, "--no-baselines": False},
    "topk16": {**COMMON, "--no-baselines": False},
    "keys16": {**COMMON, "--no-baselines": False, "--out": None},
    "rows16": {**SPREAD, "--baseline-lib": None, "--no-torch": False},
    "kth": {**SPREAD, "--baseline-lib": None, "--torch-reps": 3},
    "kth16": {**SPREAD, "--baseline-lib": None, "--torch-reps": 3},
    "kth_multi": {**SPREAD, "--baseline-lib": None},
    "kth16_multi": {**SPREAD, "--baseline-lib": None},
    "topk16_filter": {**SPREAD, "--baseline-lib": None, "--modes": "perrow_k,uniform_k,perrow_rank"},
    "topp16_filter": {**SPREAD, "--baseline-lib": None, "--check-rows": 256},
    "sample16": {**SPREAD, "--check-rows": 256},
    "temper16": {**SPREAD, "--parent-lib": None, "--gate1-rounds": 0, "--check-rows": 256},
    "logprob16": {**SPREAD, "--case": None, "--check-rows": 256},
    "unique": {**ROUNDS, "--variant": None},
    "reduce_by_key": {**ROUNDS, "--op": None},
}
ONCE = ("def one(", "def timed(", "def measure(", "def verdict(", "def spread_of(", "def bound_library(", "def bytes_per_key(",
        "def parser(", "def run_cases(", "5.5e12", "ctypes.CDLL(")
GONE = ("torch.cuda.Event", "elapsed_time(", "def one(", "def timed(", "def measure(", "def verdict(", "def baseline_library(",
        "def parent_library(", "ctypes.CDLL(", "5.5e12")


def tool_path(name):
    return os.path.join(TOOLS, name + "_perf.py")


@pytest.fixture
def clock(monkeypatch):
    """perfkit.one replaced: the n-th call returns n ms; it runs prepare and fn like the real one, so that they log themselves"""
    ticks = []

    def one(fn, prepare=None):
        if prepare:
            prepare()
        fn()
        ticks.append(float(len(ticks) + 1))
        return ticks[-1]

    monkeypatch.setattr(perfkit, "one", one)
    return ticks


def logged_sides(log):
    return {"a": lambda: log.append("a"), "base": lambda: log.append("base")}


def test_measure_spread_repeats_family(clock):
    log = []
    medians = perfkit.measure(logged_sides(log), {"base"}, repeats=3, reps=2, warmup=1, fresh=lambda: log.append("fresh"))
    assert log == ["fresh", "a", "base"] * 3 + ["fresh", "base"] * 6
    # the clock: repeat 0  a 1 3 5, base 2 4 6 (1 and 2 are warm-up);  repeat 1  base 7 8 9;  repeat 2  base 10 11 12
    assert medians == {"a": [4.0], "base": [5.0, 8.5, 11.5]}


def test_measure_rounds_family(clock):
    log = []
    medians = perfkit.measure(logged_sides(log), None, repeats=3, reps=2, warmup=1, fresh=lambda: log.append("fresh"))
    assert log == ["fresh", "a", "base"] * 9
    # repeat 0  a 1 3 5, base 2 4 6;  repeat 1  a 7 9 11, base 8 10 12;  repeat 2  a 13 15 17, base 14 16 18
    assert medians == {"a": [4.0, 10.0, 16.0], "base": [5.0, 11.0, 17.0]}


def test_measure_order_per_repeat(clock):
    log = []
    medians = perfkit.measure(logged_sides(log), None, repeats=3, reps=2, warmup=1, fresh=lambda: log.append("fresh"),
                              order=lambda repeat: ["a", "base"] if repeat % 2 == 0 else ["base", "a"])
    assert log == ["fresh", "a", "base"] * 3 + ["fresh", "base", "a"] * 3 + ["fresh", "a", "base"] * 3
    # repeat 1  base 7 9 11, a 8 10 12
    assert medians == {"a": [4.0, 11.0, 16.0], "base": [5.0, 10.0, 17.0]}


def test_measure_prepare_runs_before_its_side_alone(clock):
    log = []
    perfkit.measure(logged_sides(log), {"base"}, repeats=1, reps=1, warmup=0, prepare={"a": lambda: log.append("prepare a")})
    assert log == ["prepare a", "a", "base"]


def test_one_keeps_prepare_outside_the_events(monkeypatch):
    log = []

    class Event:
        def __init__(self, enable_timing):
            assert enable_timing

        def record(self):
            log.append("record")

        def elapsed_time(self, other):
            return 1.25

    monkeypatch.setattr(perfkit.torch.cuda, "Event", Event)
    monkeypatch.setattr(perfkit.torch.cuda, "synchronize", lambda: log.append("synchronize"))
    assert perfkit.one(lambda: log.append("fn"), lambda: log.append("prepare")) == 1.25
    assert log == ["prepare", "synchronize", "record", "fn", "record", "synchronize"]
    del log[:]
    perfkit.one(lambda: log.append("fn"))
    assert log == ["synchronize", "record", "fn", "record", "synchronize"]


def test_timed_spread_verdict_and_bytes(clock):
    log = []
    assert perfkit.timed(lambda: log.append("fn"), lambda: log.append("fresh"), reps=3, warmup=2) == (4.0, 3.0)   # of 3 4 5
    assert log == ["fresh", "fn"] * 5
    assert perfkit.timed(lambda: None, None, reps=1, warmup=0) == (6.0, 6.0)
    assert perfkit.spread_of([3.0, 1.0, 2.0]) == (2.0, 2.0)
    assert perfkit.verdict(1.0, 2.0, 0.5) == "ahead"
    assert perfkit.verdict(2.0, 1.0, 0.5) == "behind"
    assert perfkit.verdict(1.75, 2.0, 0.5) == "within spread"
    assert perfkit.verdict(1.5, 2.0, 0.5) == "within spread" and perfkit.verdict(2.5, 2.0, 0.5) == "within spread"   # equal to it
    assert perfkit.bytes_per_key(2.0, 1 << 20) == 2.0e-3 * 5.5e12 / (1 << 20)


def test_bound_library_binds_the_named_entries_alone():
    from lsdradixsort_amd import _lib

    names = ("lsdsort_topk16_workspace_bytes", "lsdsort_topk16_device", "lsdsort_check_device")
    L = perfkit.bound_library(_lib.PRODUCT_LIB, names)
    assert L is not _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        if name in names:
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        else:
            assert fn.argtypes is None, name
    with pytest.raises(KeyError):
        perfkit.bound_library(_lib.PRODUCT_LIB, ("lsdsort_no_such_entry",))
    assert perfkit.bound_library(None, names) is _lib.lib()


def test_one_definition():
    kit = open(os.path.join(TOOLS, "perfkit.py")).read()
    for text in ONCE:
        assert kit.count(text) == 1, text
    for name in OPTIONS:
        text = open(tool_path(name)).read()
        for gone in GONE:
            assert gone not in text, (name, gone)
        assert re.search(r"^import perfkit$", text, flags=re.M), name


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_command_line_did_not_move(name, capsys):
    import torch

    spec = importlib.util.spec_from_file_location(name + "_perf", tool_path(name))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert not torch.cuda.is_initialized(), "importing the tool touched the device"
    ap = tool.parser()
    got = {s: action.default for action in ap._actions for s in action.option_strings if s not in ("-h", "--help")}
    assert got == OPTIONS[name]
    with pytest.raises(SystemExit) as stop:
        ap.parse_args(["--help"])
    assert stop.value.code == 0
    assert "Usage: python tools/" + name + "_perf.py" in capsys.readouterr().out


# ---------------------------------------------------------------- tools/ab.py against a stand-in for bench.py

STAND_IN = """import json, os, sys, time
open(os.environ["AB_LOG"], "a").write(os.environ["AB_SIDE"] + " " + " ".join(sys.argv[1:]) + "\\n")
mode = os.environ.get("AB_MODE", "full")
if mode == "fail": sys.exit(3)
if mode == "sleep": time.sleep(60)
result = {"value": 1.5, "ms_per_step": 2.5, "stages_ms": {"histogram": 0.25, "scatter_per_pass": 0.5}, "config": {}}
if mode == "full": result["stages_ms"]["local_stage"], result["config"]["tile_keys"] = 0.75, 4096
print("some progress line")
print(json.dumps(result))
if mode == "empty": print()
"""


def run_ab(tmp_path, b_mode, *more):
    bench, log = tmp_path / "stand_in.py", tmp_path / "runs.log"
    bench.write_text(STAND_IN)
    cmd = [sys.executable, os.path.join(TOOLS, "ab.py"), "--rounds", "2", "--bench", str(bench), "--common", "--full --steps 2",
           "--side", "a", f"AB_SIDE=a AB_LOG={log}", "--side", "b", f"AB_SIDE=b AB_LOG={log} AB_MODE={b_mode} --pairs", *more]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    return done, log.read_text().splitlines()


def test_ab_interleaves_and_prints_the_columns(tmp_path):
    done, runs = run_ab(tmp_path, "bare")
    assert done.returncode == 0, done.stderr
    assert runs == ["a --full --steps 2", "b --full --steps 2 --pairs"] * 2
    assert done.stdout.splitlines() == ["a 1.5 2.5 0.25 0.5 4096 0.75", "b 1.5 2.5 0.25 0.5"] * 2


@pytest.mark.parametrize("b_mode,status", [("fail", "status 3"), ("empty", "status 0"), ("sleep", "status timeout")])
def test_ab_stops_at_the_first_failure(tmp_path, b_mode, status):
    done, runs = run_ab(tmp_path, b_mode, "--timeout", "1" if b_mode == "sleep" else "30")   # the sleeper alone runs into its limit
    assert done.returncode != 0
    assert len(runs) == 2 and runs[1].startswith("b "), runs
    assert done.stdout.splitlines() == ["a 1.5 2.5 0.25 0.5 4096 0.75"]
    assert "b: bench.py failed" in done.stderr and status in done.stderr


def test_ab_runs_a_side_in_its_directory(tmp_path):
    bench, log = tmp_path / "stand_in.py", tmp_path / "runs.log"
    bench.write_text(STAND_IN)   # a relative --bench: every side's own
    cmd = [sys.executable, os.path.join(TOOLS, "ab.py"), "--rounds", "1", "--bench", "stand_in.py", "--side", "tree",
           f"@{tmp_path} AB_SIDE=tree AB_LOG={log}"]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert done.returncode == 0 and done.stdout.split()[0] == "tree", done.stderr
