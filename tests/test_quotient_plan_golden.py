"""CPU: the quotient planner (csrc/quotient_plan.hip) makes, for a fixed set of constraint systems under every knob setting, exactly the
plans recorded in tests/golden/quotient_plans.json -- SHA-256 of zk_host_quotient_plan's full summary and of every class program, as
tools/quotient_plan_digest.py prints them.  The record was written by the library before the planner became its own translation unit, so
this pins the class programs bit for bit across changes that are meant to move or tighten the planner only.  (The remainder programs of
the additive split are not in the summary beyond their count: the GPU proof tests cover them.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import quotient_plan_digest as qd  # noqa: E402


@pytest.fixture(scope="module")
def blobs():
    return qd.circuits()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "quotient_plans.json")) as f:
        return json.load(f)


def test_the_record_covers_every_circuit_and_knob_setting(blobs, golden):
    assert list(golden) == [f"{label}|{name}" for label, _ in qd.KNOBS for name in blobs]
    assert len(qd.KNOBS) == 12 and len(blobs) == 9      # unset; ten single settings; DAG=0 with GROUP=0


@pytest.mark.parametrize("label,kv", qd.KNOBS, ids=[label for label, _ in qd.KNOBS])
def test_plans_equal_the_record(blobs, golden, monkeypatch, label, kv):
    """the knobs are read per plan request, so one process serves every setting (ZK_LOOKUP_PLAIN included)"""
    for name in qd.KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in kv.items():
        monkeypatch.setenv(name, value)
    got = qd.digests(blobs, label)
    assert got == {key: golden[key] for key in got}
