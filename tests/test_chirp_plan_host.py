"""gsdr_chirp_lockin_plan (csrc/chirp_plan.h through host_logic.cpp): the rule by which launch_chirp_lockin and
launch_chirp_multi_lockin choose between the plain, the split and the generic lock-in, against a table written out here
and against the invariants the split kernels rely on.  No GPU.

The table holds what the rule gave before it became one function (two copies, one per launcher), with the 16384 partial
sums a handle allocates: it pins the rule, so a change to it has to change this file."""
import ctypes as C

import pytest

PLAIN, SPLIT, GENERIC = 0, 1, 2
CAP = 16384                     # kChirpPartials of csrc/demod_state.h


def plan(lib, steps, length, ppt, index0, valid, chirps, split=1, cap=CAP):
    parts, per_part = C.c_int(-7), C.c_int(-7)
    form = lib.gsdr_chirp_lockin_plan(steps, length, ppt, index0, valid, chirps, split, cap, C.byref(parts), C.byref(per_part))
    return form, parts.value, per_part.value


def layouts(total):
    """(length, decim) with decim * ceil(length / 256) == total: one sample per step, and -- where total allows --
    steps of two and of three stretches"""
    out = [(1, total), (256, total)]
    if total % 2 == 0:
        out += [(257, total // 2), (512, total // 2)]
    if total % 3 == 0:
        out.append((600, total // 3))
    return out


# (total stretches, valid, chirps) -> (parts, per_part)
TABLE = [
    ((15, 1, 1), (1, 15)),          # fewer than 16 stretches: never split
    ((16, 1, 1), (4, 4)),           # the smallest split: four waves of four stretches
    ((18, 1, 1), (4, 5)),           # a short last part (5, 5, 5, 3)
    ((16, 512, 1), (4, 4)),         # the most points that split
    ((16, 513, 1), (1, 16)),
    ((64, 512, 1), (8, 8)),         # ~4096 waves in the launch
    ((64, 512, 16), (2, 32)),       # the partial-sum buffer exactly full: 512 * 2 * 16
    ((260, 1, 1), (65, 4)),         # more than 64 parts: the sum kernel's second round of lanes
    ((4096, 4, 1), (1024, 4)),
    ((4096, 4, 16), (256, 16)),     # the buffer again: 4 * 256 * 16
    ((18, 2, 5), (4, 5)),
]


@pytest.mark.parametrize("key,want", TABLE, ids=["total%d_valid%d_chirps%d" % k for k, _ in TABLE])
def test_plan_table(gsdr_lib, key, want):
    total, valid, chirps = key
    for length, decim in layouts(total):
        for steps, index0 in ((1000, 0), (1000, 7 * length), (3, 2 * length), (1, 0)):
            got = plan(gsdr_lib, steps, length, length * decim, index0, valid, chirps)
            assert got == ((SPLIT if want[0] > 1 else PLAIN),) + want, (key, length, decim, steps, index0, got)
            # GSDR_CHIRP_SPLIT=0, or no partial-sum buffer: a wave per point
            assert plan(gsdr_lib, steps, length, length * decim, index0, valid, chirps, split=0) == (PLAIN, 1, total)
            assert plan(gsdr_lib, steps, length, length * decim, index0, valid, chirps, cap=0) == (PLAIN, 1, total)


def test_generic_conditions(gsdr_lib):
    L = gsdr_lib
    # the table's split shape, to see that every condition below overrides it
    assert plan(L, 1000, 600, 3600, 0, 1, 1) == (SPLIT, 4, 5)
    # length: 2^23 - 1 is the last the fast kernels take (one step, so that the period stays small)
    assert plan(L, 1, (1 << 23) - 1, (1 << 23) - 1, 0, 1, 1)[0] == SPLIT
    assert plan(L, 1, 1 << 23, 1 << 23, 0, 1, 1) == (GENERIC, 1, 0)
    # period = num_steps * length: 2^32 - 2 is the last (2 * a prime: no sweep has it), 2^32 - 1 = 3 * 1431655765
    assert plan(L, (1 << 30) - 1, 4, 64, 0, 1, 1) == (SPLIT, 4, 4)              # period 2^32 - 4
    assert plan(L, 1431655765, 3, 48, 0, 1, 1) == (GENERIC, 1, 0)                # period 2^32 - 1, by the period alone
    assert plan(L, 4294967295, 1, 16, 0, 1, 1) == (GENERIC, 1, 0)
    assert plan(L, 1 << 31, 2, 32, 0, 1, 1) == (GENERIC, 1, 0)                   # period 2^32
    assert plan(L, 1_000_000, 4300, 4300, 0, 100, 2) == (GENERIC, 1, 0)          # 4.3e9
    assert plan(L, 1_000_000, 6000, 6000, 0, 3, 1) == (GENERIC, 1, 0)            # CHIRP_CASES' 64-bit rows
    # num_steps alone: 2^31 - 2 is the last (length 1)
    assert plan(L, (1 << 31) - 2, 1, 16, 0, 1, 1) == (SPLIT, 4, 4)
    assert plan(L, (1 << 31) - 1, 1, 16, 0, 1, 1) == (GENERIC, 1, 0)
    # points that are not whole steps, or do not start on a step boundary
    assert plan(L, 1000, 600, 3601, 0, 1, 1) == (GENERIC, 1, 0)
    assert plan(L, 1000, 600, 3000 + 300, 0, 1, 1) == (GENERIC, 1, 0)
    assert plan(L, 1000, 600, 3600, 1, 1, 1) == (GENERIC, 1, 0)
    assert plan(L, 1000, 600, 3600, 599, 1, 1) == (GENERIC, 1, 0)
    assert plan(L, 1000, 600, 3600, 600, 1, 1) == (SPLIT, 4, 5)
    # ... whatever the split switch says
    assert plan(L, 1000, 600, 3600, 1, 1, 1, split=0) == (GENERIC, 1, 0)
    assert plan(L, 1 << 31, 2, 32, 0, 1, 1, split=0) == (GENERIC, 1, 0)


def test_refused_arguments(gsdr_lib):
    L = gsdr_lib
    for args in ((0, 1, 16, 0, 1, 1), (10, 0, 16, 0, 1, 1), (1 << 62, 4, 16, 0, 1, 1), (10, 1, 0, 0, 1, 1), (10, 1, 16, 0, 0, 1),
                 (10, 1, 16, 0, 1, 0), (10, 1, 16, 0, 1, 17), (10, 1, 1 << 31, 0, 1, 1)):
        assert plan(L, *args)[0] == -1, args
    assert plan(L, 10, 1, 16, 0, 1, 1, cap=-1)[0] == -1
    # the two outputs are optional
    assert L.gsdr_chirp_lockin_plan(10, 1, 16, 0, 1, 1, 1, CAP, None, None) == SPLIT


def test_plan_invariants(gsdr_lib):
    """Every (total, valid, chirps) with total <= 300, valid <= 600, chirps in {1, 5, 16}: the parts cover the point,
    none is empty (chirp_lockin_split_kernel and chirp_multi_lockin_kernel would write a zero for it, which is right but
    wasted), the partial sums fit the buffer, and a split is what the rule says it is."""
    fn = gsdr_lib.gsdr_chirp_lockin_plan
    parts, per_part = C.c_int(), C.c_int()
    pp, pq = C.byref(parts), C.byref(per_part)
    seen = {PLAIN: 0, SPLIT: 0}
    for chirps in (1, 5, 16):
        for total in range(1, 301):
            for valid in range(1, 601):
                form = fn(1000, 1, total, 0, valid, chirps, 1, CAP, pp, pq)
                p, q = parts.value, per_part.value
                assert form in (PLAIN, SPLIT), (total, valid, chirps, form)
                seen[form] += 1
                assert p * q >= total and (p - 1) * q < total, (total, valid, chirps, p, q)
                assert valid * p * chirps <= CAP or form == PLAIN, (total, valid, chirps, p, q)
                if form == SPLIT:
                    assert p >= 2 and q >= 4 and total >= 16 and valid <= 512, (total, valid, chirps, p, q)
                    assert valid * p <= 4096 + valid, (total, valid, p)          # ~4096 waves
                else:
                    assert (p, q) == (1, total)
    assert seen[PLAIN] > 0 and seen[SPLIT] > 0
    # a layout with several stretches per step gives the same plan as length 1 with the same total
    for total, valid, chirps in ((18, 1, 1), (48, 7, 5), (300, 512, 16), (12, 1, 1)):
        want = fn(1000, 1, total, 0, valid, chirps, 1, CAP, pp, pq), parts.value, per_part.value
        for length, decim in layouts(total):
            assert plan(gsdr_lib, 1000, length, length * decim, 0, valid, chirps) == want, (total, length)
