"""One device allocation that holds every buffer of a launch, for the tests that put an output flush against an input.

The buffers are carved out of one uint8 tensor at byte offsets, so their distances are exact whatever the allocator does,
with a guard band before the first and behind the last.  The whole allocation is compared after the launch with what was
uploaded plus the outputs the reference expects: an output is right, an input is what it was, and no guard, gap or stride
padding has changed, each reported under its own name."""
import numpy as np

FILL = 0xA5          # every byte nobody put anything in
GUARD = 256          # bytes before the first and behind the last buffer
GAP = 64             # bytes, at the least, between two groups


def place(sizes, groups, shift=None, align=16):
    """Byte offsets {name: offset} and the slab's size.  sizes {name: bytes}; groups is a sequence of tuples of names: the
    buffers of a group lie flush against each other in the order given, groups lie GAP bytes or more apart.  A group starts
    on an `align`-byte boundary (16; a multiple of it for a test that places buffers inside a 256-byte line) plus
    shift[its first name] bytes."""
    assert align % 16 == 0 and GUARD % 16 == 0
    offsets, cursor = {}, GUARD
    for group in groups:
        cursor = -(-cursor // align) * align + (shift or {}).get(group[0], 0)
        for name in group:
            offsets[name] = cursor
            cursor += sizes[name]
        cursor += GAP
    assert sorted(offsets) == sorted(sizes), "every buffer goes into exactly one group"
    return offsets, cursor - GAP + GUARD


class Slab:
    def __init__(self, sizes, groups, shift=None, align=16):
        self.sizes, self.align = dict(sizes), align
        self.offsets, self.nbytes = place(sizes, groups, shift, align)
        self.image = np.full(self.nbytes, FILL, np.uint8)        # what the device holds before the launch
        self.dev = None

    def put(self, name, array, into=None):
        """the bytes of a host array, which fill the buffer"""
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert raw.size == self.sizes[name], (name, raw.size, self.sizes[name])
        image = self.image if into is None else into
        image[self.offsets[name]:self.offsets[name] + raw.size] = raw

    def upload(self, torch, device):
        """One allocation with `align` spare bytes, sliced to a start on an `align`-byte boundary: a buffer's address is
        that boundary plus its offset, whatever the allocator returned."""
        raw = torch.empty(self.nbytes + self.align, dtype=torch.uint8, device=device)
        start = -raw.data_ptr() % self.align
        self.dev = raw[start:start + self.nbytes]
        self.dev.copy_(torch.from_numpy(self.image))
        assert self.dev.data_ptr() % self.align == 0
        return self

    def at(self, name):
        """the buffer as a device uint8 tensor: its data_ptr() is the buffer's first byte"""
        return self.dev[self.offsets[name]:self.offsets[name] + self.sizes[name]]

    def check(self, outputs, where=""):
        """outputs {name: expected host array}; everything else must be as uploaded"""
        got = self.dev.cpu().numpy()
        want = self.image.copy()
        for name, array in outputs.items():
            self.put(name, array, into=want)
        for name, off in self.offsets.items():                               # by name first, for a message that says where
            n = self.sizes[name]
            kind = "output" if name in outputs else "input"
            assert np.array_equal(got[off:off + n], want[off:off + n]), f"{where}: {kind} {name} differs from " + \
                ("the reference" if name in outputs else "what was uploaded")
        assert (got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all(), f"{where}: a guard band was written"
        assert np.array_equal(got, want), f"{where}: bytes between the buffers were written"
