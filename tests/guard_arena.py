"""Guard-band arena for the footprint tests (tests/test_gpu_footprint.py): every operand of a call is an exact-size contiguous slice of
ONE allocation, with a band of pattern words before and after it, as a caller that carves its buffers out of one arena has them.  A store
a few words or a few polynomials past an operand then lands in a band (or in a neighbour) instead of the allocator's padding, and
check() sees it.

    ar = GuardArena(np.uint64, device=True, seed=7, odd=False)
    ar.take("acc", acc_words, written=True, guard=trailing_guard(n, ppb))   # numpy input, or a word count for an output
    ar.take("lhs", lhs_words)
    ar.take("ws", ws_bytes // 8, written=True, aligned=True)           # a workspace: its content is the call's, its bands are not
    ar.build()
    plan.mul_accumulate_batch(ar["acc"], ar["lhs"], ar["lhs"])
    got = ar.check()["acc"]            # asserts every band and every read-only operand, returns the written slices

The pattern is splitmix64(seed + word index) (its high half for 32-bit words): position dependent, so a shifted or repeated copy of a
band does not pass for the band.  Slices start 16-byte aligned, or (odd=True) one word past a 16-byte boundary: the least alignment the
word type itself promises (include/cntt.h, "Operands")."""
import numpy as np

MIN_GUARD_POLYS = 64   # a trailing band never holds fewer polynomials than this


def splitmix64(x):
    """splitmix64 of a uint64 array (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def pattern(count, seed, dtype):
    v = splitmix64(np.arange(count, dtype=np.uint64) + np.uint64(seed))
    return v if np.dtype(dtype) == np.uint64 else (v >> np.uint64(32)).astype(np.uint32)


def trailing_guard(n, ppb, words_per_coeff=1):
    """words behind a written operand of polynomials of n coefficients served by a kernel that puts `ppb` polynomials in one workgroup:
    one full workgroup's worth, and never fewer than MIN_GUARD_POLYS polynomials -- an idle slot whose store lost its mask still lands
    inside the arena"""
    return max(int(ppb), MIN_GUARD_POLYS) * n * words_per_coeff


class GuardArena:
    def __init__(self, dtype, device, seed, odd=False, align=16):
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.uint32), np.dtype(np.uint64))
        self.device, self.seed, self.odd, self.align = device, int(seed), odd, align
        self._specs, self._slices, self._built = [], {}, False

    # -- layout ----------------------------------------------------------------------------------------------------------------------
    def take(self, name, data, written=False, guard=None, lead=None, aligned=False):
        """Reserve a slice: `data` is its initial content (a numpy array of the word type) or a word count (the slice starts as pattern
        words, which a call that only writes it must replace).  guard / lead: words of the band behind / in front of it (None: 256).
        aligned: start on a 16-byte boundary even in an odd arena (a workspace, which the headers want 16-byte aligned)."""
        assert not self._built and name not in [s[0] for s in self._specs]
        if isinstance(data, (int, np.integer)):
            words, init = int(data), None
        else:
            init = np.ascontiguousarray(data).view(self.dtype).ravel().copy()
            words = init.size
        self._specs.append((name, words, init, written, 256 if guard is None else int(guard), 256 if lead is None else int(lead), aligned))
        return self

    def build(self):
        isz = self.dtype.itemsize
        step = self.align // isz                     # words per alignment unit
        # worst case: every slice start rounded up by one unit plus one word
        total = sum(w + g + l + step + 1 for (_, w, _, _, g, l, _) in self._specs) + step
        host = np.empty(total + step, dtype=self.dtype)
        if self.device:
            import torch
            self._t = torch.empty(total + step, dtype=torch.int64 if isz == 8 else torch.int32, device="cuda")
            base = self._t.data_ptr()
        else:
            self._t = host
            base = host.ctypes.data
        assert base % isz == 0
        cur = 0
        for (name, words, init, written, guard, lead, aligned) in self._specs:
            start = cur + lead
            # first word index at or after `start` whose address is 0 (aligned) or one word (odd) past a multiple of `align`
            want = isz if self.odd and not aligned else 0
            while (base + start * isz) % self.align != want:
                start += 1
            self._slices[name] = (start, words, written, init)
            cur = start + words + guard
        self.total = cur
        assert cur <= total + step
        self.pattern = pattern(self.total, self.seed, self.dtype)
        expect = self.pattern.copy()
        for name, (start, words, written, init) in self._slices.items():
            if init is not None:
                expect[start:start + words] = init
        self._before = expect
        if self.device:
            import torch
            self._t = self._t[:self.total]
            self._t.copy_(torch.from_numpy(expect.view(np.int64 if isz == 8 else np.int32)))
            torch.cuda.synchronize()
        else:
            host[:self.total] = expect
            self._t = host[:self.total]
        self._built = True
        return self

    # -- the slices --------------------------------------------------------------------------------------------------------------------
    def __getitem__(self, name):
        start, words, _, _ = self._slices[name]
        return self._t[start:start + words]

    def snapshot(self):
        if self.device:
            import torch
            torch.cuda.synchronize()
            return self._t.cpu().numpy().view(self.dtype)
        return np.array(self._t, copy=True)

    # -- the check ---------------------------------------------------------------------------------------------------------------------
    def _where(self, idx):
        prev = "the head of the arena"
        for name, (start, words, written, _) in sorted(self._slices.items(), key=lambda kv: kv[1][0]):
            if idx < start:
                return "band between %s and operand %s (%d words before it)" % (prev, name, start - idx)
            if idx < start + words:
                return "read-only operand %s, word %d" % (name, idx - start)
            prev = "operand %s" % name
            last_end = start + words
        return "band behind %s (%d words past its end)" % (prev, idx - last_end + 1)

    def check(self, unchanged=()):
        """Assert that every band word and every operand not marked `written` holds what build() put there, byte for byte; operands named
        in `unchanged` are written operands this call must nevertheless leave alone.  Returns {name: numpy copy} of the written slices."""
        assert self._built
        now = self.snapshot()
        want = self._before.copy()
        out = {}
        for name, (start, words, written, _) in self._slices.items():
            if written:
                out[name] = now[start:start + words].copy()
                if name not in unchanged:
                    want[start:start + words] = now[start:start + words]
        if now.tobytes() != want.tobytes():
            bad = np.nonzero(now != want)[0]
            i = int(bad[0])
            raise AssertionError("%d words outside the call's outputs changed; the first is arena word %d: %s (0x%x -> 0x%x); the last is word "
                                 "%d: %s" % (bad.size, i, self._where(i), int(want[i]), int(now[i]), int(bad[-1]), self._where(int(bad[-1]))))
        return out
