"""The bookkeeping of refilled batched generation (Engine.generate_batch(refill=...)): which rows wait, which slot of the decoder is free,
which slice of the cross K|V cache is free, prepared or being read. Pure Python, no torch and no device: generation.py drives the device
from its answers, tests/test_refill_generation_cpu.py drives it with hand-made finish orders.

A SLOT is a row of the one fused decoder of the call (position, input, draws, self-attention cache, log rows). A SLICE holds the cross K|V of
one prompt; there are more slices than slots, so the next waiting prompts are prepared (encoder pass, projections, prefill) AHEAD into free
slices while every slot is busy. A row goes: waiting -> prepared (owns a slice) -> live (owns a slot too) -> finished (both released).
Rows are prepared and admitted in row order, each into the lowest free slice / slot."""
from collections import deque


class RefillSchedule:
    def __init__(self, rows, slots, slices):
        if not (slots >= 1 and slices >= slots and rows >= 0):
            raise ValueError('RefillSchedule: %d rows, %d slots, %d slices' % (rows, slots, slices))
        self.rows, self.slots, self.slices = rows, slots, slices
        self.waiting = deque(range(rows))          # not prepared yet, row order
        self.ready = deque()                       # (row, slice): prepared, no slot yet, row order
        self.slice_row = [None] * slices           # the row that owns the slice (prepared or live)
        self.slot_row = [None] * slots             # the live row of the slot
        self.slot_slice = [None] * slots
        self.admitted = []                         # rows in the order they got a slot
        self.finished = 0

    def free_slot(self):
        """The lowest free slot, or None."""
        return next((s for s, r in enumerate(self.slot_row) if r is None), None)

    def free_slice(self):
        """The lowest free slice, or None."""
        return next((c for c, r in enumerate(self.slice_row) if r is None), None)

    def prepare(self):
        """The next waiting row gets the lowest free slice: (row, slice), or None when no row waits or every slice is owned. The caller
        enqueues the row's encoder pass, projections and prefill into that slice."""
        c = self.free_slice()
        if c is None or not self.waiting:
            return None
        r = self.waiting.popleft()
        self.slice_row[c] = r
        self.ready.append((r, c))
        return r, c

    def admit(self):
        """The first prepared row gets the lowest free slot: (row, slot, slice), or None when no row is prepared or no slot is free."""
        s = self.free_slot()
        if s is None or not self.ready:
            return None
        r, c = self.ready.popleft()
        self.slot_row[s], self.slot_slice[s] = r, c
        self.admitted.append(r)
        return r, s, c

    def finish(self, slot):
        """The slot's row has stopped: its slot and its slice are free again. Returns (row, slice)."""
        r, c = self.slot_row[slot], self.slot_slice[slot]
        if r is None:
            raise ValueError('RefillSchedule.finish: slot %d is empty' % slot)
        self.slot_row[slot] = self.slot_slice[slot] = None
        self.slice_row[c] = None
        self.finished += 1
        return r, c

    def done(self):
        return self.finished == self.rows
