"""What the pointer-form tests (test_recon_ptrs_gpu.py, test_update_ptrs_gpu.py) share: an arena,
one device byte buffer filled with a seeded random guard pattern, from which every shard is carved
at a chosen byte offset.  The placement order is shuffled, so addresses are not monotonic in the
shards' keys, the gaps are not uniform, and at least 16 guard bytes separate two shards.  After a
call the WHOLE arena is compared with the expected one: the written bytes, the buffers that are only
read, the guards, and nothing written for an entry that has no buffer.

Alignment classes (of the byte offsets; the arena itself is 256-byte aligned):
  A16  every buffer at a multiple of 16
  A4   as A16, but the buffer `odd` at 4 mod 16
  A1   as A16, but the buffer `odd` at one element past a multiple of 16: an odd address for
       1-byte symbols, 2 mod 4 for 2-byte symbols"""
import numpy as np


class Arena:
    def __init__(self, sizes, w, cls="A16", odd=None, seed=0):
        """sizes: {key: elements}; w: bytes per element; odd: the key of the misaligned buffer."""
        assert cls in ("A16", "A4", "A1") and (cls == "A16") == (odd is None)
        assert odd is None or odd in sizes
        rng = np.random.default_rng(seed)
        order = list(sizes)
        rng.shuffle(order)
        self.w, self.sizes, self.off = w, dict(sizes), {}
        cur = 0
        for k in order:
            cur += 16 + 16 * int(rng.integers(0, 4))            # the guard before the buffer
            cur = (cur + 15) & ~15
            self.off[k] = cur + (0 if k != odd else 4 if cls == "A4" else w)
            cur = self.off[k] + sizes[k] * w
        self.host = rng.integers(0, 256, cur + 32, dtype=np.uint8)
        for k in sizes:                                         # what the class promises
            want = 0 if k != odd else 4 if cls == "A4" else w
            assert self.off[k] % 16 == want
        spans = sorted((o, o + sizes[k] * w) for k, o in self.off.items())
        assert all(b[0] - a[1] >= 16 for a, b in zip(spans, spans[1:])) and spans[0][0] >= 16

    def put(self, host, key, values):
        """Write the elements `values` of buffer `key` into the host image `host` of the arena."""
        v = np.ascontiguousarray(values)
        assert v.itemsize == self.w and v.size == self.sizes[key]
        host[self.off[key]:self.off[key] + v.size * self.w] = v.view(np.uint8).reshape(-1)

    def get(self, host, key, dtype):
        o = self.off[key]
        return host[o:o + self.sizes[key] * self.w].copy().view(dtype)

    def upload(self, torch, host):
        dev = torch.from_numpy(host.copy()).cuda()
        assert dev.data_ptr() % 256 == 0
        return dev

    def tensor(self, torch, dev, key):
        """The device tensor of buffer `key`: a view into the arena `dev`."""
        o = self.off[key]
        t = dev[o:o + self.sizes[key] * self.w]
        return t if self.w == 1 else t.view(torch.uint16)


def download(dev):
    return dev.cpu().numpy()
