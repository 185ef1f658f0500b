"""CPU: the launch plan of the quotient evaluator (csrc/quotient_lower.hpp: plan_quotient_launch, seen through zk_host_quotient_launch) -- the
kernel, the accumulator's home, the slices, the LDS size, the region sizes and every word of the program region zk_quotient_eval uploads --
over the programs and knob settings of the device tests (quotient_programs.corpus() x SETTINGS, sliceable_corpus() x SLICE_SETTINGS), for
packed columns and for coset records.

Every expectation is restated here from what the kernels need (csrc/quotient.hip):
  * k_quotient_eval2 reads 4-word instructions, word 3 the class mask of word 0 (class_mask below restates the table; with record operands a
    sum or difference with a memory operand takes the forms that read the operand where it arrived); k_quotient_eval reads 3-word ones;
  * both fetch instructions two ahead and the memory operand one ahead: four END records follow every stream;
  * k_quotient_eval2 keeps one stack entry in registers, k_quotient_eval two; the rest is in LDS, nine limbs x 256 lanes x 4 bytes an entry;
  * FULL means the grid covers the domain exactly: 2^ext_k >= 256;
  * a sliced launch maps workgroups 8 j + x, j = t S .. t S + S - 1, to the S slices of one row tile: the number of row tiles must be a multiple
    of 8 and only k_quotient_eval2 has the slice table; a slice starts from acc = 0 with its own parking slots, and the combining program
    acc = acc * k_s + P_s reads the slices' sums as columns behind the parked intermediates;
  * the accumulator lives in memory where a fold is rare (16 folds <= instructions), never in a sliced launch;
  * the stream of a (sub-)program is what zk_host_quotient_lower gives for it (quotient_programs.fuse_of names the `fuse` of a setting), with
    K_FIRST_FOLD on its first fold.
quotient_programs.variant() / setting_streams(), the restatement the device tests' coverage assertion rests on, is held against the plan too."""
import random

import pytest

import quotient_programs as qp
from quotient_programs import (Q_ADD, Q_ADD_CONST, Q_DOUBLE, Q_FOLD, Q_MUL, Q_MUL_CONST, Q_NEG, Q_PUSH_COL, Q_PUSH_CONST, Q_PUSH_TMP, Q_SQUARE, Q_SUB,
                               Q_TEE_TMP, K_ADD_COL, K_SUB_COL, K_RSUB_COL, K_MUL_COL, K_FOLD_COL, K_MAC_COL)
from zkevm_circuits_amd import binding

K_PUSH_COL32, K_MAC2_COL, K_MAC_STK = 23, 24, 25
K_FIRST_FOLD, K_ANY_FLAG = 0x4000, 0x100 | 0x200 | 0x400 | 0x800 | 0x1000 | 0x2000
THREADS, LIMBS = 256, 9

# one bit per step of k_quotient_eval2's loop body
(C_SPILL, C_UNPACK_T, C_UNPACK_B, C_UNPACK_B32, C_POP_B, C_HASMEM, C_FLAGS, C_MULV, C_MULC, C_ADDV, C_SUBV, C_FOLDC, C_RARE, C_PUSHC, C_ADDC, C_RSUB, C_MULS,
 C_NEG, C_SQ, C_DBL, C_TEE, C_FOLD, C_MACC, C_UNPACK_T32, C_MAC2, C_MACS, C_ADDM, C_SUBM) = (1 << i for i in range(28))
CLASS = {Q_PUSH_COL: C_SPILL | C_UNPACK_T | C_HASMEM, Q_PUSH_CONST: C_SPILL | C_RARE | C_PUSHC, Q_ADD: C_POP_B | C_ADDV, Q_SUB: C_POP_B | C_RARE | C_RSUB,
         Q_MUL: C_POP_B | C_RARE | C_MULS, Q_NEG: C_RARE | C_NEG, Q_SQUARE: C_RARE | C_SQ, Q_DOUBLE: C_RARE | C_DBL, Q_FOLD: C_RARE | C_FOLD, Q_MUL_CONST: C_MULC,
         Q_ADD_CONST: C_RARE | C_ADDC, Q_TEE_TMP: C_RARE | C_TEE, K_ADD_COL: C_UNPACK_B | C_HASMEM | C_ADDV, K_SUB_COL: C_UNPACK_B | C_HASMEM | C_SUBV,
         K_RSUB_COL: C_UNPACK_B | C_HASMEM | C_RARE | C_RSUB, K_MUL_COL: C_UNPACK_B32 | C_HASMEM | C_MULV, K_FOLD_COL: C_UNPACK_B | C_HASMEM | C_FOLDC,
         K_MAC_COL: C_UNPACK_B32 | C_HASMEM | C_MACC, K_MAC2_COL: C_UNPACK_B32 | C_HASMEM | C_MAC2, K_MAC_STK: C_POP_B | C_RARE | C_MACS}


def class_mask(w0, records):
    op = w0 & 0xff
    if op == K_PUSH_COL32:           # its flags belong to the entry it spills: no flag step of its own
        return C_UNPACK_T32 | C_HASMEM
    if records and op in (K_ADD_COL, K_SUB_COL):
        m = C_HASMEM | (C_ADDM if op == K_ADD_COL else C_SUBM)
    else:
        m = CLASS.get(op, 0)         # NOP, END: nothing
    return m | (C_FLAGS if w0 & K_ANY_FLAG else 0)


def is_fold(w0):
    return (w0 & 0xff) in (Q_FOLD, K_FOLD_COL)


def streams_of(plan):
    """the plan's words taken apart: [(first word, [instruction tuples])] per stream, checking the END records and everything behind the streams"""
    w, wpi, S = plan["words"], plan["words_per_instr"], plan["S"]
    assert len(w) * 4 == plan["prog_bytes"]
    if plan["sliced"]:
        tab = w[plan["slice_tab_at"]:]
        assert len(tab) == 2 * S                                       # the slice table ends the region
        spans = [(tab[2 * s], tab[2 * s + 1] - 1) for s in range(S)]      # (first word, instructions + 1: the END counts as one)
    else:
        assert S == 1
        spans = [(0, plan["low_len"])]
    at, out = 0, []
    for first, n in spans:
        assert first == at                                             # streams back to back
        out.append([tuple(w[first + wpi * i:first + wpi * (i + 1)]) for i in range(n)])
        assert all((ins[0] & 0xff) != 0 for ins in out[-1])
        at = first + wpi * (n + 4)
        assert w[first + wpi * n:at] == [0] * (4 * wpi)               # four END records (opcode 0, empty class mask)
    assert plan["comb_at"] == at
    if plan["sliced"]:
        comb = [tuple(w[at + 4 * s:at + 4 * (s + 1)]) for s in range(S)]
        assert w[at + 4 * S:at + 4 * S + 16] == [0] * 16
        assert plan["slice_tab_at"] == at + 4 * S + 16
    else:
        comb = []
        assert plan["slice_tab_at"] == at and w[at:] == [0] * (4 * wpi)      # room the upload reserves and leaves zero
    return out, comb


def caller_cuts(prog, streams):
    """where the caller's program was cut: the lowering turns each FOLD into one FOLD or FOLD_COL, so slice s ends behind as many of the
    caller's folds as streams 0 .. s hold"""
    fold_pos = [pc + 1 for pc, (op, a, b) in enumerate(prog) if op == Q_FOLD]
    cuts, done = [0], 0
    for st in streams:
        done += sum(is_fold(ins[0]) for ins in st)
        cuts.append(fold_pos[done - 1])
    assert cuts[-1] == len(prog)
    return cuts


def renumbered(prog, cuts):
    """the slices as programs of their own: cut only where the stack is empty, parking slots numbered per slice out of one range"""
    out, nxt = [], 0
    for x, y in zip(cuts, cuts[1:]):
        assert qp.stack_depth(prog[x:y]) >= 0                          # asserts that the slice leaves the stack empty
        slot_of, sub = {}, []
        for op, a, b in prog[x:y]:
            if op == Q_TEE_TMP and a not in slot_of:
                slot_of[a], nxt = nxt, nxt + 1
            sub.append((op, slot_of[a], b) if op in (Q_TEE_TMP, Q_PUSH_TMP) else (op, a, b))      # KeyError: read of a value parked outside the slice
        out.append(sub)
    return out, nxt


def check_plan(case, env, records, cuts32=None):
    """every field and word of the plan of `case` under the knobs `env` (in force), restated; returns the plan and the caller's cut points"""
    prog, ncols, nconsts, ne = case.prog, case.ncols, case.nconsts, 1 << case.ext_k
    plan = binding.host_quotient_launch(prog, ncols, nconsts, case.ext_k, records)
    v2 = env.get("ZK_QUOTIENT_KERNEL") != "1"
    wpi = 4 if v2 else 3
    assert plan["kernel"] == (2 if v2 else 1) and plan["words_per_instr"] == wpi and plan["records"] == records
    assert plan["full"] == (ne >= THREADS)
    if plan["sliced"]:
        assert v2 and ((ne // THREADS) & 7) == 0 and plan["S"] >= 2
    streams, comb = streams_of(plan)
    assert sum(len(st) for st in streams) == plan["low_len"]
    # the streams: the lowering of the (sub-)programs
    if plan["sliced"]:
        cuts = caller_cuts(prog, streams)
        subs, num_tmp = renumbered(prog, cuts)
        fuse = qp.fuse_of({k: v for k, v in env.items() if k != "ZK_QUOTIENT_FUSE"})       # a slice is lowered whatever ZK_QUOTIENT_FUSE says
    else:
        cuts, subs, fuse = [], [prog], qp.fuse_of(env)
        num_tmp = 1 + max([a for op, a, b in prog if op == Q_TEE_TMP], default=-1)
    assert plan["num_tmp"] == num_tmp
    depth, folds = 1, 0
    for sub, st in zip(subs, streams):
        words, d = qp.lower(sub, ncols, fuse)
        want = [tuple(int(x) for x in words[3 * i:3 * i + 3]) for i in range(len(words) // 3)]
        first = next((i for i, ins in enumerate(want) if is_fold(ins[0])), None)
        if first is not None:
            want[first] = (want[first][0] | K_FIRST_FOLD,) + want[first][1:]
        assert [ins[:3] for ins in st] == want
        assert sum(bool(ins[0] & K_FIRST_FOLD) for ins in st) == (first is not None)
        if v2:
            assert [ins[3] for ins in st] == [class_mask(ins[0], records) for ins in st]
        depth = max(depth, d)
        folds += sum(is_fold(ins[0]) for ins in st)
    assert plan["depth"] == depth and plan["folds"] == folds
    assert plan["lds"] == max(depth - (1 if v2 else 2), 1) * LIMBS * THREADS * 4
    assert plan["acc_in_mem"] == (not plan["sliced"] and folds > 0 and 16 * folds <= plan["low_len"])
    # the combining program and the regions behind the program
    S = plan["S"]
    for s, ins in enumerate(comb):
        w0 = K_FOLD_COL | ((nconsts + s) << 16) | (0 if s else K_FIRST_FOLD)
        assert ins == (w0, ncols + num_tmp + s, 0, class_mask(w0, False))          # the slices' sums are packed elements whatever the operands are
    extra = S if plan["sliced"] else 0
    assert plan["col_bytes"] == max(ncols + num_tmp + extra, 1) * 8
    assert plan["const_bytes"] == max(nconsts + extra, 1) * 64 * 2                 # nine limbs in a 64-byte record, R and R' forms
    assert plan["tile_alias"] == 0
    if cuts32 is not None:
        assert cuts == cuts32
    return plan, cuts


def check_mirror(case, env, plan):
    """quotient_programs.variant / setting_streams (packed columns) against the plan's head record"""
    v = qp.variant(case.prog, case.ncols, case.ext_k, env)
    assert v == (("sliced",) if plan["sliced"] else ("v2" if plan["kernel"] == 2 else "v1", plan["full"], plan["acc_in_mem"]))
    sts = qp.setting_streams(case, env)
    assert len(sts) == plan["S"] and sum(len(w) // 3 for w in sts) == plan["low_len"]


_CORPUS = qp.corpus()
_SLICEABLE = qp.sliceable_corpus()


@pytest.mark.parametrize("setting", list(qp.SETTINGS))
def test_corpus_plans(setting):
    env = qp.SETTINGS[setting]
    with qp.knobs(env):
        for case in _CORPUS:
            plan, _ = check_plan(case, env, False, cuts32=qp.slice_cuts(case.prog, case.ext_k))
            assert not plan["sliced"]                       # ZK_QUOTIENT_SLICES unset: nothing this small is cut
            check_mirror(case, env, plan)
            if env.get("ZK_QUOTIENT_KERNEL") != "1" and 2 <= case.ext_k <= 26:
                rec, _ = check_plan(case, env, True)
                for f in ("kernel", "full", "acc_in_mem", "sliced", "S", "depth", "lds", "num_tmp", "low_len", "folds", "comb_at", "slice_tab_at", "prog_bytes"):
                    assert rec[f] == plan[f], f             # the same lowered words: only class masks differ
            else:
                with pytest.raises(binding.ZkError) as e:      # no record mode in k_quotient_eval; rows addressed with 32-bit byte offsets from 2^2 rows on
                    binding.host_quotient_launch(case.prog, case.ncols, case.nconsts, case.ext_k, True)
                assert e.value.status == -5


@pytest.mark.parametrize("slices", qp.SLICE_SETTINGS)
def test_sliceable_plans(slices):
    env = {"ZK_QUOTIENT_SLICES": slices}
    with qp.knobs(env):
        for case in _SLICEABLE:
            cuts32 = qp.slice_cuts(case.prog, case.ext_k)
            sliceable = ((1 << case.ext_k) // THREADS) & 7 == 0
            for records in (False, True):
                plan, cuts = check_plan(case, env, records, cuts32=cuts32 if sliceable else [])      # a forced count cuts alike for both row sizes
                assert plan["sliced"] == (slices != "0" and sliceable) and (not plan["sliced"] or plan["S"] == len(cuts32) - 1)
            check_mirror(case, env, binding.host_quotient_launch(case.prog, case.ncols, case.nconsts, case.ext_k, False))
        # a slice is lowered with the fused steps whatever ZK_QUOTIENT_FUSE says, and without them under ZK_QUOTIENT_MAC=0
        for extra in ({"ZK_QUOTIENT_FUSE": "0"}, {"ZK_QUOTIENT_MAC": "0"}, {"ZK_QUOTIENT_MAC": "1"}, {"ZK_QUOTIENT_RELAXED": "0"}):
            with qp.knobs(dict(env, **extra)):
                check_plan(_SLICEABLE[0], dict(env, **extra), True)


def test_only_kernel_2_slices_and_only_row_tiles_in_multiples_of_eight():
    case = _SLICEABLE[0]
    with qp.knobs({"ZK_QUOTIENT_SLICES": "3", "ZK_QUOTIENT_KERNEL": "1"}):
        assert not check_plan(case, {"ZK_QUOTIENT_SLICES": "3", "ZK_QUOTIENT_KERNEL": "1"}, False)[0]["sliced"]
    with qp.knobs({"ZK_QUOTIENT_SLICES": "3"}):
        for ext_k, sliced in ((10, False), (11, True), (12, True)):        # 4 row tiles; 8; 16
            small = qp.Case("sliceable", case.prog, ext_k, ext_k, False)
            assert check_plan(small, {"ZK_QUOTIENT_SLICES": "3"}, False)[0]["sliced"] == sliced


def test_a_record_launch_is_cut_for_36_byte_rows():
    """ZK_QUOTIENT_SLICES unset: the slices wanted are the operands of the rows in flight (every distinct column x the row size x min(2^ext_k,
    327 680) rows) over 96 MiB, rounded up -- 96 columns at 2^16 rows are 192 MiB packed (2 slices) and 216 MiB as records (3)."""
    rng = random.Random(20261020)
    prog = qp.sliceable_program(rng, 96, 4, 700)
    case = qp.Case("sliceable96", prog, 16, 16, False)
    assert len(prog) >= 2048 and case.ncols == 96 and len({a for op, a, b in prog if op == Q_PUSH_COL}) == 96
    want = lambda row_bytes: -(-(96 * row_bytes * (1 << 16)) // (96 << 20))
    assert (want(32), want(36)) == (2, 3)
    with qp.knobs({}):
        cuts32 = qp.slice_cuts(prog, 16)
        packed, cuts_p = check_plan(case, {}, False, cuts32=cuts32)
        rec, cuts_r = check_plan(case, {}, True)
    assert packed["sliced"] and rec["sliced"] and (packed["S"], rec["S"]) == (2, 3)
    assert cuts_r != cuts32 and len(cuts_r) == 4


def test_programs_the_evaluator_refuses():
    def status(prog, ncols, nconsts, ext_k, records=False):
        with pytest.raises(binding.ZkError) as e:
            binding.host_quotient_launch(prog, ncols, nconsts, ext_k, records)
        return e.value.status
    with qp.knobs({}):
        deep = qp.deep_case(17, 8, 8)
        assert status(deep.prog, deep.ncols, deep.nconsts, 8) == -5                      # stack deeper than 16
        ok = qp.deep_case(16, 8, 8)
        assert binding.host_quotient_launch(ok.prog, ok.ncols, ok.nconsts, 8)["depth"] <= 16
        assert status([(Q_PUSH_COL, 3, 0), (Q_FOLD, 0, 0)], 3, 1, 8) == -1               # column out of range
        assert status([(Q_PUSH_COL, 0, 0), (Q_FOLD, 1, 0)], 1, 1, 8) == -1               # constant out of range
        assert status([(Q_PUSH_COL, 0, 0), (Q_ADD, 0, 0), (Q_FOLD, 0, 0)], 1, 1, 8) == -1   # stack underflow
        assert status([(Q_PUSH_TMP, 0, 0), (Q_FOLD, 0, 0)], 1, 1, 8) == -1               # read before it is parked
        assert status([(Q_PUSH_COL, 0, 0), (Q_FOLD, 0, 0)], 1, 1, 27, records=True) == -5   # record rows are addressed with 32-bit byte offsets
    with qp.knobs({"ZK_QUOTIENT_SLICES": "2"}):
        case = _SLICEABLE[0]
        assert binding.host_quotient_launch(case.prog, case.ncols, (1 << 16) - 3, case.ext_k)["sliced"]
        assert status(case.prog, case.ncols, (1 << 16) - 2, case.ext_k) == -5            # the combining program names constant num_consts + s in 16 bits
