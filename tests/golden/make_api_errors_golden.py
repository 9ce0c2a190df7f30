"""Writes tests/golden/api_errors.json: return code and mpcq_last_error() text of every case of tests/api_error_cases.py, from the library
given (the lane emulator's by default).  The golden is the characterisation a change of the C ABI's host code is held to, so it is made
with the library of the commit BEFORE such a change: check that commit out somewhere, build its emulator (make -C tests/wave_emu) and run

    python tests/golden/make_api_errors_golden.py path/to/that/libmpcq_emu.so

from this tree (the case table is this tree's)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from api_error_cases import run_cases  # noqa: E402

if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(HERE), "wave_emu", "libmpcq_emu.so")
    got = run_cases(lib)
    with open(os.path.join(HERE, "api_errors.json"), "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(got)} cases, {sum(1 for v in got.values() if v['rc'] == 0)} of them succeed, from {lib}")
