"""The evaluation cache's definition in numpy (csrc/nn/eval_cache.h states it in C++, the kernels of
csrc/nn/eval_cache.hip run it): the two row hashes, the tag, the slot, and CacheModel -- which rows of
which call hit, and which entries exist afterwards, as a serial program.  The reference for tests."""
import numpy as np

from galvanise_zero_amd.util.symmetry import pick_hashes

MAX_CHUNK_ROWS = 2048
_M64 = (1 << 64) - 1


def _bits(X):
    X = np.ascontiguousarray(X, dtype=np.float32)
    return X.reshape(X.shape[0], -1).view(np.uint32)


def _mix32b(x):
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x2c1b3c6d)
    x = x ^ (x >> np.uint32(12))
    x = x * np.uint32(0x297a2d39)
    return x ^ (x >> np.uint32(15))


def hash1(X):
    """The first row hash: csrc/nn/symmetry.h's pick_hash as it stands.  uint32 [n]."""
    return pick_hashes(X)


def hash2(X):
    """The second: sum over i of mix32b(b_i + 0x85EBCA77 * (i + 1)) mod 2^32.  uint32 [n]."""
    bits = _bits(X)
    with np.errstate(over="ignore"):
        k = np.uint32(0x85EBCA77) * np.arange(1, bits.shape[1] + 1, dtype=np.uint32)
        return _mix32b(bits + k[None, :]).sum(axis=1, dtype=np.uint32)


def tags(X):
    """tag = h2 << 32 | h1.  uint64 [n]."""
    return (hash2(X).astype(np.uint64) << np.uint64(32)) | hash1(X).astype(np.uint64)


def mix64(x):
    x = int(x) & _M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def slots(X, entries):
    """slot = mix64(tag) % entries, for any entries >= 1.  Python ints [n]."""
    return [mix64(t) % int(entries) for t in tags(X)]


def tag_mask(tag_bits):
    return _M64 if tag_bits >= 64 else 0 if tag_bits <= 0 else (1 << tag_bits) - 1


def claim_word(seq, row):
    return (seq << 16) | (~row & 0xFFFF)


class CacheModel(object):
    """CacheModel(entries, tag_bits, chunk_rows).call(X) -> the hit mask of that call (int32 [n]), the
    table updated as the kernels update it: a call goes through in chunks of chunk_rows rows, all rows
    of a chunk are probed before any is inserted, and of the missed rows that map to one slot the
    lowest inserts (a later chunk over an earlier one).  A hit needs the masked tag and all plane
    words equal, so tag_bits filters and the planes decide.  Counts as gz_eval_cache_stats."""

    def __init__(self, entries, tag_bits=64, chunk_rows=MAX_CHUNK_ROWS):
        self.entries = int(entries)
        self.mask = tag_mask(tag_bits)
        self.chunk = min(int(chunk_rows), MAX_CHUNK_ROWS) if chunk_rows and chunk_rows > 0 else MAX_CHUNK_ROWS
        self.table = {}          # slot -> (tag, key bytes); a flush empties it
        self.claim = {}          # slot -> claim word (survives a flush, as on the device)
        self.seq = 0
        self.calls = self.rows = self.hits = self.forward_rows = self.inserts = self.replaced = self.flushes = 0

    def flush(self):
        self.table = {}
        self.flushes += 1

    def probe(self, X):
        """The hit mask without side effects."""
        bits = _bits(X)
        out = np.zeros(bits.shape[0], dtype=np.int32)
        for r, (t, s) in enumerate(zip(tags(X), slots(X, self.entries))):
            e = self.table.get(s)
            out[r] = int(e is not None and ((e[0] ^ int(t)) & self.mask) == 0 and e[1] == bits[r].tobytes())
        return out

    def call(self, X):
        bits = _bits(X)
        n = bits.shape[0]
        hit = np.zeros(n, dtype=np.int32)
        tg, sl = [int(t) for t in tags(X)], slots(X, self.entries)
        for r0 in range(0, n, self.chunk):
            c = min(self.chunk, n - r0)
            self.seq += 1
            hit[r0:r0 + c] = self.probe(bits[r0:r0 + c].view(np.float32))
            missed = [r for r in range(c) if not hit[r0 + r]]
            for r in missed:
                s = sl[r0 + r]
                self.claim[s] = max(self.claim.get(s, 0), claim_word(self.seq, r))
            for r in missed:
                s = sl[r0 + r]
                if self.claim[s] != claim_word(self.seq, r):
                    continue
                self.inserts += 1
                self.replaced += int(s in self.table)
                self.table[s] = (tg[r0 + r], bits[r0 + r].tobytes())
        if n:
            self.calls += 1
        self.rows += n
        self.hits += int(hit.sum())
        self.forward_rows += n - int(hit.sum())
        return hit

    def digest(self):
        """The valid entries as one number: sum of mix64(tag ^ mix64(slot + 1)) mod 2^64."""
        return sum(mix64(t ^ mix64(s + 1)) for s, (t, _) in self.table.items()) & _M64
