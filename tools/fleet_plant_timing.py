"""Device time of fleet_plant_kernel (every quadrotor its own plant, csrc/mpcq_fleet.hpp) next to plant_kernel (the engine's shared plant),
whose place it takes in a period while a fleet is set.

Runs tools/microbench/fleet_plant (built from fleet_plant.hip with the line in its header if it is missing): both kernels from the
library's own headers, launched as the engine launches them, alternately in one process, every launch between a HIP-event pair of its
own, `--launches` timed launches each after 20 warm-up launches, at the plant update of the bench workload (2 substeps of 5 ms) and --
for the kernel's scaling with the substep count -- at a control period of 0.1 s (20 substeps).  A report, not a gate.

usage: python tools/fleet_plant_timing.py [--out profiles/fleet_plant_timing.json] [--batches 1024,8192] [--launches 200]
"""
import argparse
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "microbench", "fleet_plant.hip")
EXE = os.path.join(HERE, "microbench", "fleet_plant")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "--offload-arch=gfx950", "-std=c++17", "-fno-strict-aliasing",
                               "-o", EXE, SRC])
    out = {"tool": "tools/fleet_plant_timing.py", "runs": []}
    for n_sub in (2, 20):
        txt = subprocess.check_output([EXE, str(n_sub), "5e-3", str(args.launches)] + args.batches.split(","), text=True)
        for line in txt.splitlines():
            out["runs"].append(json.loads(line))
            print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
