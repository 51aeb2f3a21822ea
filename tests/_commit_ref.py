"""The numpy reference of the commitment kernels (csrc/merkle.hip), written from the definition on canonical words: the overwrite-mode
sponge of a row, the binary tree, the mixed-height tree of a segment commitment (oracle/stark_segment.inc `MixedTree::build`) and the
FRI leaves. The permutation is tests/_poseidon2_air_ref.permute (vectorised plain `% p`); `constants` = (ext_rc[8][16], int_rc[13],
diag[16]) canonical, as prover.poseidon2_constants() and sm.poseidon2_constants() return them. tests/test_commit_ref_cpu.py ties every
function to the oracle."""
import numpy as np

from tests._poseidon2_air_ref import permute

RATE, DIGEST = 8, 8


def _permute(states, constants):
    return permute(states, constants)[0]


def sponge(rows, constants):
    """rows: [n, W] canonical words, W >= 1 -> [n, 8] digests: the state starts at 0, each block of 8 words OVERWRITES the first words
    of the state and is followed by a permutation; a short last block keeps the words it does not overwrite"""
    rows = np.asarray(rows, dtype=np.uint32)
    n, W = rows.shape
    assert W >= 1
    st = np.zeros((n, 16), np.uint32)
    for c0 in range(0, W, RATE):
        block = rows[:, c0:c0 + RATE]
        st[:, :block.shape[1]] = block
        st = _permute(st, constants)
    return st[:, :DIGEST].copy()


def compress(left, right, constants):
    """[n, 8], [n, 8] -> [n, 8]: the first 8 words of permute(left || right)"""
    return _permute(np.concatenate([np.asarray(left, np.uint32), np.asarray(right, np.uint32)], axis=1), constants)[:, :DIGEST].copy()


def binary_tree(leaves, constants):
    """leaves: [n, 8], n a power of two -> the (2n - 1) * 8 words of all levels, leaves first, root last (prover_internal.hpp "Digest
    tree layout"): parent i = compress(child 2i, child 2i + 1)"""
    level = np.asarray(leaves, dtype=np.uint32).reshape(-1, DIGEST)
    n = len(level)
    assert n >= 1 and n & (n - 1) == 0
    out = [level]
    while len(level) > 1:
        level = compress(level[0::2], level[1::2], constants)
        out.append(level)
    return np.concatenate(out).reshape(-1)


def mixed_tree(matrices, constants):
    """matrices: [[height, width] canonical], heights powers of two, in AIR order -> the (2N - 1) * 8 words of the levels of N = the
    largest height, N / 2, ..., 1 nodes (the device layout of merkle_commit_mixed): level N = the sponge of the concatenated rows of
    the matrices of height N; node j of the level of n < N nodes = compress(child j, child j + n), then, where matrices of height n
    exist, compress(node, sponge of their concatenated rows j)"""
    mats = [np.asarray(m, dtype=np.uint32) for m in matrices]
    N = max(len(m) for m in mats)
    assert all(len(m) & (len(m) - 1) == 0 for m in mats)

    def rows_of(n):
        here = [m for m in mats if len(m) == n]
        return sponge(np.concatenate(here, axis=1), constants) if here else None

    level = rows_of(N)
    out = [level]
    n = N >> 1
    while n >= 1:
        level = compress(level[:n], level[n:], constants)
        inject = rows_of(n)
        if inject is not None:
            level = compress(level, inject, constants)
        out.append(level)
        n >>= 1
    return np.concatenate(out).reshape(-1)


def ext_pair_leaves(v, constants):
    """v: [2 * half, 4] extension elements -> [half, 8]: leaf i = permute(v[i] || v[i + half] || 0^8)[:8]"""
    v = np.asarray(v, dtype=np.uint32).reshape(-1, 4)
    half = len(v) // 2
    assert len(v) == 2 * half
    return _permute(np.concatenate([v[:half], v[half:], np.zeros((half, 8), np.uint32)], axis=1), constants)[:, :DIGEST].copy()
