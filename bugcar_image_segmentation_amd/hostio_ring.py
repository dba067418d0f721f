"""Bookkeeping of hostio.HostStream's slot ring: which slot the next put uses, which step the next
fetch returns, how many steps are outstanding, and the overrun / underrun errors. Pure Python (no
torch, no native library), so it is tested without a GPU (tests/test_hostio_ring.py).

Steps are numbered 0, 1, 2, ... in put order and fetched in the same order (FIFO); step k lives in
slot k % depth. A slot may be put again only once its previous step has been fetched, which with
FIFO fetching is the same as: at most `depth` steps are outstanding.
"""
from __future__ import annotations


class SlotRing:
    def __init__(self, depth: int):
        if int(depth) != depth or depth < 1:
            raise ValueError("depth must be an integer >= 1")
        self.depth = int(depth)
        self._put = 0          # steps put so far = the next put's sequence number
        self._got = 0          # steps fetched so far = the next fetch's sequence number

    @property
    def outstanding(self) -> int:
        return self._put - self._got

    @property
    def full(self) -> bool:
        return self.outstanding == self.depth

    @property
    def put_slot(self) -> int:
        """The slot the next put() will use (whether or not it is free yet)."""
        return self._put % self.depth

    def put(self) -> tuple[int, int]:
        """Claim the next slot: (slot, sequence number). RuntimeError if that slot's previous step
        has not been fetched."""
        if self.full:
            raise RuntimeError(f"overrun: slot {self.put_slot} still holds the unfetched result of step "
                               f"{self._put - self.depth} ({self.depth} steps outstanding; get() first)")
        seq = self._put
        self._put += 1
        return seq % self.depth, seq

    def peek(self) -> tuple[int, int]:
        """(slot, sequence number) of the oldest unfetched step. RuntimeError if there is none."""
        if self.outstanding == 0:
            raise RuntimeError("underrun: no step is outstanding (put() first)")
        return self._got % self.depth, self._got

    def get(self) -> tuple[int, int]:
        """Release the oldest unfetched step: (slot, sequence number)."""
        slot, seq = self.peek()
        self._got += 1
        return slot, seq
