"""What the TIFF paths share between a file and the device: the two pinned staging buffers a reader or writer takes in turn (a pair
per caller: a running read and a running write share no buffer) and the groups in which a raster's streams are worked through."""
import torch

GROUP_BYTES = 256 << 20


class PinnedPair:
    """Two pinned byte buffers, kept between calls and grown by a quarter beyond what is asked for.  A slot may be marked busy until
    the copy out of it has passed (``copied``); ``take`` waits for that."""

    def __init__(self):
        self.buffers, self._busy, self._turn = [None, None], [None, None], 0

    def take(self, slot, n) -> torch.Tensor:
        """slot ``slot``'s buffer, of at least n bytes, free of any earlier copy marked with ``copied``"""
        if self._busy[slot] is not None:
            self._busy[slot].synchronize()
            self._busy[slot] = None
        if self.buffers[slot] is None or self.buffers[slot].numel() < n:
            self.buffers[slot] = None
            self.buffers[slot] = torch.empty(max(n, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return self.buffers[slot]

    def take_next(self, n):
        """(buffer, slot) of the slot whose turn it is: one copy may be in flight while the other buffer is filled"""
        self._turn = 1 - self._turn
        return self.take(self._turn, n), self._turn

    def copied(self, slot):
        """call after queueing the copy out of the slot's buffer on the current stream"""
        self._busy[slot] = torch.cuda.Event()
        self._busy[slot].record()


def stream_groups(n_streams: int, tiles_x: int, stream_bytes: int, group_bytes: int):
    """(first, n) of the groups a raster's streams are worked through in: as many streams as ``group_bytes`` of raw tile bytes hold,
    whole tile rows where a row fits, one stream at least"""
    per = max(1, int(group_bytes) // stream_bytes)
    if per >= tiles_x:
        per -= per % tiles_x
    return [(first, min(per, n_streams - first)) for first in range(0, n_streams, per)]
