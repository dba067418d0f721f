"""The slot-ring bookkeeping of hostio.HostStream (hostio_ring.SlotRing), without a GPU: slot
numbering, sequence numbers, the outstanding count, and the overrun / underrun errors."""
import os
import subprocess
import sys

import pytest

from bugcar_image_segmentation_amd.hostio_ring import SlotRing


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_slots_go_round_and_sequence_numbers_increase(depth):
    r = SlotRing(depth)
    puts, gets = [], []
    for _ in range(3 * depth + 1):
        assert r.put_slot == len(puts) % depth
        puts.append(r.put())
        assert r.outstanding == 1
        gets.append(r.get())
        assert r.outstanding == 0
    assert [s for s, _ in puts] == [k % depth for k in range(len(puts))]
    assert [q for _, q in puts] == list(range(len(puts)))
    assert gets == puts                                    # FIFO: the same slot and number come back


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_overrun_raises_and_changes_nothing(depth):
    r = SlotRing(depth)
    for k in range(depth):
        assert not r.full
        assert r.put() == (k, k)
    assert r.full and r.outstanding == depth
    with pytest.raises(RuntimeError, match="overrun"):
        r.put()                                            # put number depth + 1 with no fetch in between
    assert r.outstanding == depth and r.put_slot == 0
    assert r.get() == (0, 0)                               # after a fetch that slot may be put again
    assert r.put() == (0, depth)
    with pytest.raises(RuntimeError, match="overrun"):
        r.put()
    assert [r.get() for _ in range(depth)] == [((k % depth), k) for k in range(1, depth + 1)]


def test_underrun_raises_and_changes_nothing():
    r = SlotRing(2)
    with pytest.raises(RuntimeError, match="underrun"):
        r.get()
    with pytest.raises(RuntimeError, match="underrun"):
        r.peek()
    assert r.outstanding == 0 and r.put() == (0, 0)
    assert r.peek() == (0, 0) and r.outstanding == 1       # peek does not release
    assert r.get() == (0, 0)
    with pytest.raises(RuntimeError, match="underrun"):
        r.get()
    assert r.put() == (1, 1)


def test_fetches_lag_puts_in_order():
    r = SlotRing(3)
    got = []
    for k in range(10):                                    # keep the ring full, as HostStream.map does
        if r.full:
            got.append(r.get())
        assert r.put() == (k % 3, k)
    while r.outstanding:
        got.append(r.get())
    assert got == [(k % 3, k) for k in range(10)]


@pytest.mark.parametrize("depth", [0, -1, 1.5])
def test_depth_must_be_a_positive_integer(depth):
    with pytest.raises(ValueError):
        SlotRing(depth)


def test_ring_module_needs_neither_torch_nor_the_native_library():
    code = ("import sys\n"
            "import bugcar_image_segmentation_amd.hostio_ring as m\n"
            "assert m.SlotRing(2).put() == (0, 0)\n"
            "bad = [n for n in sys.modules if n == 'torch' or n.endswith('._native')]\n"
            "assert not bad, bad\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
