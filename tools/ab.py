#!/usr/bin/env python3
"""A/B sides through bench.py, interleaved: rounds outermost, the sides in the given order within a round.  Every run is a fresh
child process under its own time limit; the last line of its output is the JSON result.  Printed per run, flushed:
  label value ms_per_step stages_ms.histogram stages_ms.scatter_per_pass [config.tile_keys] [stages_ms.local_stage]
At the first run that exits non-zero, runs out of time, prints nothing or prints no JSON, the driver says which side and what
status on stderr and exits 1 without starting anything else.  There is no retry.
A side is --side LABEL SPEC, SPEC a string of words: @DIR runs the side in that directory, VAR=value words before the first
option set its environment (LSDSORT_LIB=... selects a library variant), the rest are further bench.py arguments (a SPEC that is
one bare option needs a leading space, " --pairs", or argparse takes it for an option of the driver).
Usage: python tools/ab.py [--rounds 2] [--timeout 150] [--bench PATH] [--common "--full --steps 20 ..."] --side LABEL SPEC ...
  e.g. python tools/ab.py --side a "LSDSORT_LIB=lsdradixsort_amd/liblsdsort_a.so" --side cfg3 "--tile-config 3" --side old "@../old"
A relative --bench is looked up in each side's directory (tools/ab_trees.sh: every tree's own bench.py)."""
import argparse
import json
import os
import re
import shlex
import signal
import subprocess
import sys

COMMON = "--full --steps 20 --warmup 3 --no-cpu-baseline --no-extra"
REPO_BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")


def parse_side(label, spec):
    """(label, environment assignments, working directory or None, further bench.py arguments)"""
    env, cwd, words = {}, None, shlex.split(spec)
    while words and not words[0].startswith("-"):
        word = words.pop(0)
        if word.startswith("@"):
            cwd = word[1:]
        elif re.match(r"[A-Za-z_]\w*=", word):
            env.update([word.split("=", 1)])
        else:
            raise SystemExit(f"side {label!r}: {word!r} is neither @DIR, VAR=value nor an option")
    return label, env, cwd, words


def run_bench(bench, args, env, cwd, limit):
    """(status, stdout) of one bench.py child; status "timeout" after `limit` seconds, with the child's process group killed"""
    try:
        child = subprocess.Popen([sys.executable, bench] + args, env={**os.environ, **env}, cwd=cwd, stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, text=True, start_new_session=True)
    except OSError as e:
        return f"not started: {e}", ""
    try:
        out = child.communicate(timeout=limit)[0]
        return child.returncode, out
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.communicate()
        return "timeout", ""


def columns(d):
    s = d["stages_ms"]
    cols = [d["value"], d["ms_per_step"], s["histogram"], s["scatter_per_pass"]]
    if "tile_keys" in d.get("config", {}):
        cols.append(d["config"]["tile_keys"])
    if "local_stage" in s:
        cols.append(s["local_stage"])
    return cols


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds for each bench.py run")
    ap.add_argument("--bench", default=REPO_BENCH)
    ap.add_argument("--common", default=COMMON, help="arguments of every bench.py run")
    ap.add_argument("--side", nargs=2, action="append", required=True, metavar=("LABEL", "SPEC"))
    a = ap.parse_args(argv)
    sides = [parse_side(label, spec) for label, spec in a.side]
    for _ in range(a.rounds):
        for label, env, cwd, extra in sides:
            status, out = run_bench(a.bench, shlex.split(a.common) + extra, env, cwd, a.timeout)
            last = out.splitlines()[-1].strip() if out else ""
            try:
                if status != 0 or not last:
                    raise ValueError("no result")
                cols = columns(json.loads(last))
            except (ValueError, KeyError, TypeError):
                print(f"{label}: bench.py failed (status {status}, last line {last[:200]!r}), stopping", file=sys.stderr)
                return 1
            print(label, *cols, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
