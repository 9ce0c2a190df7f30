"""Device time of sensor_kernel (noise, bias, latency and dropout per quadrotor, csrc/mpcq_sensor.hpp) alone.

Runs tools/microbench/sensor (built from sensor.hip with the line in its header if it is missing): the kernel from the library's own
header, launched as the engine launches it, every launch between a HIP-event pair of its own, `--launches` timed launches after 20
warm-up launches, with every channel on (all four Philox calls, six logarithms and sincos per lane, the ring read) and, alternating with
it in the same process, with all-zero sensors (the identity: no draw), for ring depths 1 and 8.  A report, not a gate.

usage: python tools/sensor_timing.py [--out profiles/sensor_timing.json] [--batches 1024,8192] [--depths 1,8] [--launches 200]
"""
import argparse
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "microbench", "sensor.hip")
EXE = os.path.join(HERE, "microbench", "sensor")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--depths", default="1,8")
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "--offload-arch=gfx950", "-std=c++17", "-fno-strict-aliasing",
                               "-o", EXE, SRC])
    out = {"tool": "tools/sensor_timing.py", "runs": []}
    for depth in args.depths.split(","):
        txt = subprocess.check_output([EXE, depth, str(args.launches)] + args.batches.split(","), text=True)
        for line in txt.splitlines():
            out["runs"].append(json.loads(line))
            print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
