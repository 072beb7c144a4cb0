"""ngsUtf8Decode and ngsPackResults each keep a grow-only scan scratch per (device, stream). Both are
driven here on ONE stream with nothing waiting in between: decode 300 strings, pack 300 rows, decode
5,000, pack 5,000, one synchronise at the end. If the two calls shared a buffer, or one replaced a
buffer that queued work still reads, a scan would run over another's tile states. Each result is
compared with the host references of test_gpu_utf8.py and test_gpu_pack.py.
"""
import numpy as np
import pytest

from test_gpu_pack import Block, make_counts, make_values
from test_gpu_utf8 import FILL, GUARD, ref_batch
from utf8_ref import random_strings

import stringsearchlib_amd as ssl

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


class Decode:
    """The buffers of one ngsUtf8Decode call and its expected result."""

    def __init__(self, strings):
        self.strings, self.n = strings, len(strings)
        flat = b"".join(strings) + b"\x80\x80\x80"
        offs = np.cumsum([0] + [len(s) for s in strings], dtype=np.int64)
        self.cap = 4 * int(offs[-1])
        self.raw = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV)
        self.off = torch.from_numpy(offs).to(DEV)
        self.out = torch.full((self.cap + GUARD + 4,), FILL, dtype=torch.uint8, device=DEV)
        self.out_off = torch.full((self.n + 1,), -1, dtype=torch.int64, device=DEV)

    def queue(self, stream):
        ssl.utf8_decode_device(self.raw.data_ptr(), self.off.data_ptr(), self.n, self.out.data_ptr(), self.cap,
                               self.out_off.data_ptr(), stream)

    def check(self, where):
        counts, units = ref_batch(self.strings)
        ob = self.out.cpu().numpy()
        got = ob[:self.cap].view("<u4").astype(np.int64)
        assert np.array_equal(self.out_off.cpu().numpy(), 4 * np.concatenate([[0], np.cumsum(counts)])), where
        assert np.array_equal(got[:len(units)], units), where
        assert (ob[self.cap:self.cap + GUARD] == FILL).all(), f"{where}: wrote past the capacity"


def _block(n, stride, seed):
    rng = np.random.default_rng(seed)
    keys, bits = make_values(n, stride, rng)
    return Block(make_counts("random", n, stride, rng), keys, bits, n, stride)


def test_decode_and_pack_alternate_on_one_stream_without_waiting():
    steps = [("decode 300", Decode(random_strings(300, 71))), ("pack 300", _block(300, 9, 72)),
             ("decode 5000", Decode(random_strings(5000, 73))), ("pack 5000", _block(5000, 9, 74))]
    torch.cuda.synchronize()  # the inputs are in place
    s = torch.cuda.Stream(DEV)
    for _, x in steps:
        if isinstance(x, Decode):
            x.queue(s.cuda_stream)
        else:
            assert x.pack(stream=s.cuda_stream) == 0
    s.synchronize()
    for where, x in steps:
        x.check(where)
