"""The numpy reference of the sparse memory Merkle tree (powdr_amd/memory_tree.py, pw_memory_tree_*): a dict per level,
one batch of tests/_poseidon2_air_ref.permute per level, only the touched paths re-hashed (the library rebuilds every level: two
routes to the same tree), the root, the record rows in the library's order, and a dense brute-force tree for small heights.

Words are canonical. Constants: prover.poseidon2_constants()."""
import numpy as np

from tests import _poseidon2_air_ref as p2

P = p2.P


def compress(pairs, constants):
    """pairs [n, 16] canonical -> [n, 8]: the first 8 words of the permutation of every row"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 16)
    if not len(pairs):
        return np.zeros((0, 8), np.uint32)
    return p2.permute(pairs, constants)[0][:, :8].astype(np.uint32)


def leaf_digests(payloads, constants):
    payloads = np.asarray(payloads, dtype=np.int64).reshape(-1, 8)
    return compress(np.concatenate([payloads, np.zeros_like(payloads)], axis=1), constants)


def zero_digests(height, constants):
    """Z_0 .. Z_height"""
    z = [leaf_digests(np.zeros((1, 8)), constants)[0]]
    for _ in range(height):
        z.append(compress(np.concatenate([z[-1], z[-1]])[None], constants)[0])
    return z


class SparseTree:
    def __init__(self, height, constants):
        self.height, self.constants = height, constants
        self.zero = zero_digests(height, constants)
        self.payload = {}                                # key -> uint32[8]
        self.levels = [dict() for _ in range(height + 1)]  # index -> uint32[8]

    def digest(self, level, index):
        return self.levels[level].get(index, self.zero[level])

    def root(self):
        return self.digest(self.height, 0)

    def write(self, keys, payloads):
        """the leaves `keys` hold `payloads`; the nodes above them are hashed again, one batch per level"""
        keys = [int(k) for k in keys]
        payloads = np.asarray(payloads, dtype=np.uint32).reshape(len(keys), 8)
        if not keys:
            return
        for k, w, d in zip(keys, payloads, leaf_digests(payloads, self.constants)):
            self.payload[k], self.levels[0][k] = w.copy(), d
        touched = sorted(set(keys))
        for l in range(1, self.height + 1):
            touched = sorted({t >> 1 for t in touched})
            pairs = np.array([np.concatenate([self.digest(l - 1, 2 * t), self.digest(l - 1, 2 * t + 1)]) for t in touched])
            for t, d in zip(touched, compress(pairs, self.constants)):
                self.levels[l][t] = d

    def mismatch(self, keys, init):
        """the smallest key whose payload (zero: not stored) is not its init row, or None"""
        init = np.asarray(init, dtype=np.uint32).reshape(len(keys), 8)
        bad = [int(k) for k, w in zip(keys, init) if (self.payload.get(int(k), np.zeros(8, np.uint32)) != w).any()]
        return min(bad) if bad else None

    def phase_rows(self, keys, phase):
        """-> (rows [m, 24]: left, right, out; ids [m] uint64 = phase << 63 | level << 56 | index): level 0 in key order, then the nodes of
        T_1 .. T_H by index"""
        rows, ids = [], []
        zero8 = np.zeros(8, np.uint32)
        touched = [int(k) for k in keys]
        for k in touched:
            rows.append(np.concatenate([self.payload.get(k, zero8), zero8, self.digest(0, k)]))
            ids.append((phase << 63) | k)
        for l in range(1, self.height + 1):
            touched = sorted({t >> 1 for t in touched})
            for t in touched:
                rows.append(np.concatenate([self.digest(l - 1, 2 * t), self.digest(l - 1, 2 * t + 1), self.digest(l, t)]))
                ids.append((phase << 63) | (l << 56) | t)
        return np.array(rows, np.uint32).reshape(-1, 24), np.array(ids, np.uint64)

    def update(self, keys, init, fin):
        """the library's update with status 0 -> (records [25, 2^log_h] canonical, ids [n_rows], log_h, n_rows)"""
        assert self.mismatch(keys, init) is None
        r0, i0 = self.phase_rows(keys, 0)
        self.write(keys, fin)
        r1, i1 = self.phase_rows(keys, 1)
        rows = np.concatenate([r0, r1])
        n = len(rows)
        log_h = max(1, (n - 1).bit_length())
        m = np.zeros((25, 1 << log_h), np.uint32)
        m[0, :n] = 1
        m[1:, :n] = rows.T
        return m, np.concatenate([i0, i1]), log_h, n


def dense_root(height, leaves, constants):
    """the root of the full tree of 2^height leaves, {key: payload} written and everything else zero: brute force"""
    payloads = np.zeros((1 << height, 8), np.uint32)
    for k, w in leaves.items():
        payloads[k] = w
    level = leaf_digests(payloads, constants)
    for _ in range(height):
        level = compress(level.reshape(-1, 16), constants)
    return level[0]
