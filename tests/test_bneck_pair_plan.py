"""The pair overlay's walk (bugseg_debug_pair_walk, host only): which consecutive fp32 C = 64 regular
bottlenecks a forward runs as one launch, and where every tensor then lives. A paired launch writes where its first
block would have, so what follows lives in the other activation buffer; a pair cut by a forward's op range runs as
plain launches through the spare buffer. The rules are restated here as a simulation of the three buffers: whatever
the plan and however a forward is cut into calls, every op must read the tensor the op before it wrote."""
import itertools
import random

import pytest

from bugcar_image_segmentation_amd import _native as N

PLAIN, PAIR, SKIP, LONE_FIRST, LONE_SECOND = range(5)


@pytest.fixture(autouse=True)
def _lib(native_lib):
    return native_lib


def _plan(kinds, h=120, w=160):
    """ops reading and writing the two activation buffers in turn; kinds[k]: 'c' a candidate on the h x w grid,
    'C' one on another grid, '.' any other op"""
    return [(k in "cC", h if k != "C" else h // 2, w if k != "C" else w // 2, (i + 1) & 1, i & 1) for i, k in enumerate(kinds)]


ENET = "..cccc." + "." * 16 + ".cc..."      # init, down 1, 1.1-1.4, down 2, stages 2-3, up 4, 4.1, 4.2, up 5, 5.1, classes


def _enet_plan():
    p = _plan(ENET)
    n = len(p)
    # the decoder's last six ops keep their row-windowed launches: not candidates
    return [(ok and i < n - 6, h, w, a, b) for i, (ok, h, w, a, b) in enumerate(p)]


def _simulate(plan, cuts):
    """run the plan in the calls [cuts[j], cuts[j + 1]) and check every read. Tensor k is op k's output."""
    n = len(plan)
    holds = {0: None, 1: None, "spare": None}
    holds[plan[0][3]] = -1                                   # the first op's input
    for first, last in zip(cuts, cuts[1:]):
        _, acts = N.pair_walk(plan, first, last)
        k = first
        while k < last:
            act, flip = acts[k]
            src, dst = plan[k][3] ^ flip, plan[k][4] ^ flip
            if act == PAIR:
                assert acts[k + 1][0] == SKIP and k + 1 < last
                assert holds[src] == k - 1
                holds[dst] = k + 1                           # the pair's output: block k + 1's, where block k's would go
                k += 2
                continue
            assert act != SKIP, "a skipped op is reached only through its pair"
            if act == LONE_FIRST:
                dst = "spare"
            if act == LONE_SECOND:
                dst, src = src, "spare"                      # from the spare buffer to where the pair writes
            assert holds[src] == k - 1, f"op {k} reads tensor {holds[src]}"
            holds[dst] = k
            k += 1
    return holds


def test_enet_pairs_stage_1_and_leaves_the_windowed_decoder_alone():
    plan = _enet_plan()
    m, acts = N.pair_walk(plan)
    assert m == 2
    assert [a for a, _ in acts[2:6]] == [PAIR, SKIP, PAIR, SKIP]
    assert all(a == PLAIN for a, _ in acts[:2] + acts[6:])
    # the second pair and nothing else runs in the other buffers: two pairs put everything back
    assert [f for _, f in acts] == [0, 0, 0, 0, 1, 1] + [0] * (len(plan) - 6)
    _simulate(plan, [0, len(plan)])


@pytest.mark.parametrize("cut", range(1, 8))
def test_a_forward_cut_in_two_reads_what_it_wrote(cut):
    plan = _enet_plan()
    _, acts = N.pair_walk(plan, 0, cut)
    if cut in (3, 5):                                        # between the two ops of a pair
        assert acts[cut - 1][0] == LONE_FIRST and acts[cut][0] == LONE_SECOND
        assert N.pair_walk(plan, cut, len(plan))[1][cut][0] == LONE_SECOND
    whole = _simulate(plan, [0, len(plan)])
    assert _simulate(plan, [0, cut, len(plan)])[0] == whole[0] and _simulate(plan, [0, cut, len(plan)])[1] == whole[1]


def test_where_a_tensor_lives_does_not_depend_on_the_cuts():
    rng = random.Random(7)
    for _ in range(200):
        kinds = "".join(rng.choice("cccC.") for _ in range(rng.randint(1, 12)))
        plan = _plan(kinds)
        n = len(plan)
        whole = _simulate(plan, [0, n])
        for r in range(1, 4):
            for cuts in itertools.combinations(range(1, n), min(r, n - 1)):
                got = _simulate(plan, [0, *cuts, n])
                assert (got[0], got[1]) == (whole[0], whole[1]), (kinds, cuts)


def test_what_pairs_and_what_does_not():
    pairs = lambda kinds, **kw: N.pair_walk(_plan(kinds), **kw)[0]
    assert pairs("cc") == 1 and pairs("ccc") == 1 and pairs("cccc") == 2 and pairs("c.c") == 0
    assert pairs("cC") == 0 and pairs("CC") == 1             # one grid per pair
    assert pairs("") == 0 and pairs("c") == 0
    # three in a row: the first two pair, the third runs alone in the other buffer
    assert N.pair_walk(_plan("ccc"))[1] == [(PAIR, 0), (SKIP, 0), (PLAIN, 1)]
    # not the arena's ping-pong (the second op does not write the buffer the first reads): no pair
    p = _plan("cc")
    assert N.pair_walk([p[0], (True, 120, 160, p[1][3], -1)])[0] == 0
    assert N.pair_walk([(True, 120, 160, -1, 0), p[1]])[0] == 0


def test_bad_arguments_are_refused():
    for first, last in [(-1, 2), (2, 1), (0, 3)]:
        with pytest.raises(ValueError):
            N.pair_walk(_plan("cc"), first, last)
