"""CPU: the closed forms ZK_OP_EXP_ROWS computes (exp_rows_cases.closed) against the reference's serial loop restated line by line
(exp_rows_cases.assign) on every shared scenario, every column; and the facts the closed forms rest on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exp_rows_cases as ex  # noqa: E402

SCENARIOS = ex.scenarios()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_closed_forms_are_the_serial_loop(name):
    events, n = SCENARIOS[name]
    want = ex.assign(events, n, cut=not ex.fits(events, n))
    got = ex.closed(events, n)
    for col in ex.COLUMNS:
        assert got[col] == want[col], (name, col, [i for i, (a, b) in enumerate(zip(got[col], want[col])) if a != b][:5])


def test_the_reference_asserts_where_the_events_do_not_fit():
    events, n = SCENARIOS["n_cuts_an_event_midway"]
    with pytest.raises(AssertionError):
        ex.assign(events, n)


def test_step_count_and_exponents_are_exp_by_squarings():
    for base, x in [(3, 13), (23, 123), (7, ex.M256), (5, 1 << 255), (2, 2), (9, 3), (ex.RANDOM_WORD, (1 << 128) + 1)]:
        steps = []
        assert ex.exp_by_squaring(base, x, steps) == pow(base, x, 1 << 256)
        assert len(steps) == ex.steps_of(x)
        e = x
        for j, (a, b, d) in enumerate(reversed(steps)):
            assert ex.step_exponent(x, j) == e and d == pow(base, e, 1 << 256)
            assert (a, b) == ((pow(base, e - 1, 1 << 256), base) if e & 1 else (pow(base, e // 2, 1 << 256),) * 2)
            e = e // 2 if e % 2 == 0 else e - 1
        assert e == 1
    assert ex.steps_of(0) == ex.steps_of(1) == 0 and ex.steps_of(ex.M256) == 510 and ex.steps_of(1 << 255) == 255


def test_the_carries_are_exact_and_the_parity_chip_never_overflows():
    for a, b in [(ex.M256, ex.M256), (0, 5), (1, ex.M256), (1 << 255, 1 << 255), (ex.RANDOM_WORD, ex.RANDOM_WORD ^ ex.M256)]:
        d = a * b & ex.M256
        cells, _, _ = ex.muladd_witness(a, b, 0, d)
        al, bl = ex.limbs64(a), ex.limbs64(b)
        t = [sum(al[i] * bl[k - i] for i in range(k + 1)) for k in range(4)]
        carry_lo = sum(cells[3, i] << 16 * i for i in range(4)) + (cells[4, 0] << 64)
        carry_hi = sum(cells[5, i] << 16 * i for i in range(4)) + (cells[6, 0] << 64)
        assert t[0] + (t[1] << 64) == (d & ex.M128) + (carry_lo << 128)
        assert t[2] + (t[3] << 64) + carry_lo == (d >> 128) + (carry_hi << 128)
    for x in (2, 3, ex.M256, 1 << 255):
        cells, _, _ = ex.muladd_witness(2, x >> 1, x & 1, x)
        assert all(cells[5, i] == 0 for i in range(4)) and cells[6, 0] == 0


def test_scenarios_stay_small_and_cover_the_edges():
    assert all(n <= 1 << 15 for _, n in SCENARIOS.values())
    ns = {n for _, n in SCENARIOS.values()}
    assert {0, 1, 9, 10, 17, 18, 26} <= ns and any(n % 8 for n in ns)
    assert any(len(e) > 4096 for e, _ in SCENARIOS.values()) and any(len(e) == 0 for e, _ in SCENARIOS.values())
    assert any(not ex.fits(e, n) for e, n in SCENARIOS.values())
