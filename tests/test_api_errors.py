"""Return codes, mpcq_last_error() texts and the order of the argument and state checks of the C ABI, case by case against
tests/golden/api_errors.json (tests/api_error_cases.py is the table, tests/golden/make_api_errors_golden.py the generator).  The golden
was recorded from the library as it stood before the features' host code in mpcq_api.hip was gathered into one section each (Tick,
EngineView, plan_checks, replan_stage, grow_or_fail, needs_trajectories, feature_stop): whoever merges or moves a check there is held to
the same code, the same text and the same winner where a call breaks two rules at once.  No case launches the step kernel; the same table
runs on the lane emulator (CPU) and on the product library (-m gpu)."""
import json
import os
import subprocess

import pytest

from api_error_cases import CASES, run_cases

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "wave_emu")
MPCQ_ERR_INVALID, MPCQ_ERR_STATE = -1, -3

with open(os.path.join(HERE, "golden", "api_errors.json")) as fh:
    GOLDEN = json.load(fh)


def check(got):
    wrong = {cid: dict(got=got[cid], want=GOLDEN[cid]) for cid in got if got[cid] != GOLDEN[cid]}
    assert not wrong, json.dumps(wrong, indent=1)


def test_table_and_golden_match():
    ids = [cid for cid, _, _ in CASES]
    assert len(set(ids)) == len(ids)
    assert sorted(ids) == sorted(GOLDEN)
    # every case but the two that document an accepted call is an MPCQ_ERR_INVALID or MPCQ_ERR_STATE site
    ok = sorted(cid for cid, v in GOLDEN.items() if v["rc"] == 0)
    assert ok == ["mission_set/linear_ignores_bad_opts", "set_legs/without_wp_ignores_n_wp_8"]
    assert all(v["rc"] in (MPCQ_ERR_INVALID, MPCQ_ERR_STATE) and v["error"] for cid, v in GOLDEN.items() if cid not in ok)


def test_api_errors_emulator():
    subprocess.check_call(["make", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    check(run_cases(os.path.join(EMU_DIR, "libmpcq_emu.so")))


@pytest.mark.gpu
def test_api_errors_device():
    check(run_cases(None))
