#!/usr/bin/env python3
"""Interleaved A/B of another build of the library (e.g. the parent commit's, built in a checkout
of its own) against this tree's, for a change that should move nothing: plain bench.py, the
driver's call (--steps 20 --warmup 5), --config nat, --config acl_rules and tools/enqueue_bench.py,
each ROUNDS times per side, alternating; rows {"side", "run", "line"} (tools/show_ab.py) to
<outdir>/<tag>_<name>.jsonl (outdir: profiles/ by default). Any failing run ends the job.
usage: tools/ab_parent.py <parent libebpfemu.so> <tag> [outdir]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT, TAG = os.path.abspath(sys.argv[1]), sys.argv[2]
OUT = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
ROUNDS = 5
BENCH = [sys.executable, os.path.join(ROOT, "bench.py")]
SPECS = [("5tuple", BENCH), ("5tuple_driver", BENCH + ["--steps", "20", "--warmup", "5"]),
         ("nat", BENCH + ["--config", "nat"]), ("acl_rules", BENCH + ["--config", "acl_rules"]),
         ("enqueue", [sys.executable, os.path.join(ROOT, "tools", "enqueue_bench.py")])]
os.makedirs(OUT, exist_ok=True)
assert os.path.exists(PARENT)
for name, cmd in SPECS:
    path = os.path.join(OUT, f"{TAG}_{name}.jsonl")
    with open(path, "w") as f:
        for run in range(ROUNDS):
            for side in ("parent", "branch"):
                env = dict(os.environ)
                if side == "parent":
                    env["EBPFEMU_LIB_PATH"] = PARENT
                r = subprocess.run(["timeout", "-k", "10", "120"] + cmd, env=env, capture_output=True,
                                   text=True)
                line = next((l for l in r.stdout.splitlines() if l.startswith("{")), None)
                if r.returncode != 0 or line is None:
                    print(name, side, run, "exit", r.returncode, r.stdout[-1500:], r.stderr[-1500:])
                    sys.exit(1)
                d = json.loads(line)
                f.write(json.dumps({"side": side, "run": run, "line": d}) + "\n")
                f.flush()
                print(name, side, run, d.get("value"), d.get("unit"), flush=True)
