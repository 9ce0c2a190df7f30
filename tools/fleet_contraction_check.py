"""Does fleet_plant_kernel contract plant_eval into multiply-adds exactly as plant_kernel does?  (No GPU needed.)

A fleet of default plants has to integrate bit for bit as the engine's shared plant (csrc/mpcq_fleet.hpp).  Both kernels inline the same
plant_eval, but the compiler fuses multiplications and additions across statements, and where a sum of two products can be fused either
way its choice depends on the surrounding code.  This script disassembles the device code of csrc/build/api.o, rebuilds the expression
tree of every value computed in the Runge-Kutta loop of the two kernels (leaves anonymous, the two factors of a product unordered) and
checks that every derivative expression of plant_kernel's loop occurs in fleet_plant_kernel's loop with the same structure.  A necessary
condition for the identity, not a proof of it: tests/test_fleet.py (defaults are the identity) holds the identity itself on the device
and runs this check on the built object without one (test_contraction_matches_plant_kernel).  It reads the kernels by their mangled
names and takes the first loop a kernel closes as its Runge-Kutta loop: a change of either shows as an error, not as a pass.

usage: python tools/fleet_contraction_check.py [path/to/api.o]      exit status 0: same structure
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("MPCQ_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
PLANT = "_ZN4mpcq12plant_kernelIdEEvNS_8DevModelIT_EEPdPKdidi"
FLEET = "_ZN4mpcq5fleet18fleet_plant_kernelENS0_4ArgsE"
DEFAULT_OBJ = os.path.join(ROOT, "mpc_quad_ros_amd", "csrc", "build", "api.o")


def disassemble(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True).splitlines()


def inner_loop(lines, name):
    """The instructions of the kernel's innermost (first closed) loop: from the target of its first backward branch to that branch."""
    start = next(n for n, l in enumerate(lines) if re.match(r"^[0-9a-f]+ <" + re.escape(name) + ">:", l))
    ins = []
    for l in lines[start + 1:]:
        if re.match(r"^[0-9a-f]+ <", l):
            break
        m = re.match(r"\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m:
            ins.append((int(m.group(2), 16), m.group(1)))
    for addr, text in ins:
        m = re.match(r"s_cbranch_\w+ (\d+)", text)
        if m and int(m.group(1)) > 32767:
            target = addr + 4 + (int(m.group(1)) - 65536) * 4
            return [t for a, t in ins if target <= a < addr]
    raise SystemExit(f"no loop found in {name}")


def expressions(body):
    """[expression of every double-precision result of the loop, in program order]."""
    env, out = {}, []

    def val(tok):
        tok = tok.strip()
        neg = tok.startswith("-")
        tok = tok.lstrip("-").strip("|")
        e = env.get(tok) or ("L" if re.match(r"[vs]\[", tok) else tok)
        return ("-" if neg else "") + e

    for text in body:
        m = re.match(r"(v_\w+?)(?:_e32|_e64)? (.*)", text)
        if not m:
            continue
        op, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
        if op in ("v_mul_f64", "v_add_f64"):
            e = op[2:5] + "(" + ",".join(sorted([val(args[1]), val(args[2])])) + ")"
        elif op == "v_fma_f64":
            e = "fma(" + ",".join(sorted([val(args[1]), val(args[2])])) + ";" + val(args[3]) + ")"
        elif op == "v_fmac_f64":
            e = "fma(" + ",".join(sorted([val(args[1]), val(args[2])])) + ";" + val(args[0]) + ")"
        elif op == "v_cvt_f64_i32":
            e = "SIGN"
        else:
            continue
        env[args[0]] = e
        out.append(e)
    return out


def check(obj):
    """(derivative expressions of plant_kernel's loop that fleet_plant_kernel contracts differently, a one-line report)."""
    with tempfile.TemporaryDirectory() as tmp:
        lines = disassemble(obj, tmp)
    plant, fleet = expressions(inner_loop(lines, PLANT)), expressions(inner_loop(lines, FLEET))
    # the stage-point updates x + hc k of plant_kernel: fma(hc, k; x) with k a derivative expression
    updates = sorted(set(e for e in plant if e.startswith("fma(") and e.endswith(";L)") and e.count("(") > 1))
    if len(updates) < 8:   # (13 state components, some of one shape: fewer means the loop was not recognised)
        raise SystemExit(f"only {len(updates)} derivative expressions found in plant_kernel's loop: the disassembly is not what this script reads")
    everything = " ".join(fleet)
    missing = []
    for e in updates:
        k = re.sub(r"^fma\(L,|^fma\(", "", e)[:-3]
        if k not in everything:
            missing.append(k)
    return missing, (f"plant_kernel: {len(plant)} results in the loop, {len(updates)} distinct derivative expressions; "
                     f"fleet_plant_kernel: {len(fleet)} results")


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OBJ
    missing, report = check(obj)
    print(report)
    for k in missing:
        print("not in fleet_plant_kernel with this structure:", k)
    print("same multiply-add structure" if not missing else f"{len(missing)} derivative expressions are contracted differently")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
