"""The one buffer a host-packed image call uploads: the per-item descriptors, then, at a multiple of 16 bytes, one int32
table that every descriptor indexes by offsets counted in ints.  resize_frames, detector_input and resize_images pack theirs here.  numpy
only: neither the library nor a device is touched before `upload`."""
import numpy as np


class TablePacker:
    def __init__(self, *head, what='tables'):
        """head: arrays of 4-byte elements that open the table, in order (the first at offset 0); what: the table's name in a refusal"""
        self.parts, self.size, self.offsets, self.what = [], 0, {}, what
        for array in head:
            self.append(array)

    def append(self, array):
        """-> the offset (in ints) at which `array`, of 4-byte elements, now lies"""
        at, part = self.size, array.reshape(-1)
        self.parts.append(part if part.dtype == np.int32 else part.view(np.int32))
        self.size += part.size
        return at

    def _align(self, ints):
        if self.size % ints:
            self.append(np.zeros(-self.size % ints, np.int32))

    def place(self, key, *arrays, align_ints=1):
        """`arrays` end to end, once per key -> their offsets.  The group starts and ends at a multiple of align_ints: 4 keeps the tap
        tables of section 18, which lead their groups and are read as 16-byte entries, at multiples of 4 ints"""
        if key not in self.offsets:
            self._align(align_ints)
            self.offsets[key] = tuple([self.append(a) for a in arrays])
            self._align(align_ints)
        return self.offsets[key]

    def blob(self, items):
        """-> (bytes of the buffer, byte offset of the table in it, n_tables): the descriptor block is rounded up to 16 bytes, and the
        table is never empty (a call wants a table pointer), so one zero stands for none"""
        if self.size >= 2 ** 31:
            raise ValueError(f'the {self.what} of this call exceed 2^31 entries')
        items = items.view(np.uint8)                             # a contiguous 1-D array of descriptors
        at, n_tables = -(-items.size // 16) * 16, max(self.size, 1)
        blob = np.zeros(at + 4 * n_tables, np.uint8)
        blob[:items.size] = items
        if self.size:
            blob[at:at + 4 * self.size] = np.concatenate(self.parts).view(np.uint8)
        return blob, at, n_tables

    def upload(self, items, device):
        """one pinned, non-blocking copy -> (the device buffer, to be kept alive over the launch; items pointer; tables pointer; n_tables)"""
        from . import _lib
        blob, at, n_tables = self.blob(items)
        blob_d = _lib.host_to_device(blob, device)
        return blob_d, blob_d.data_ptr(), blob_d.data_ptr() + at, n_tables
