"""The reference of the memory tree's multi-opening (powdr_amd/memory_tree.py MemoryTree.open / verify_opening, pw_memory_tree_open,
pw_memory_opening_verify): a second route to the multiproof, node by node from tests/_memory_tree_ref.SparseTree.digest
and Python sets — no search in a sorted array and no scan, which is how the library finds and places the siblings — and a numpy verifier
that walks dicts of known nodes upwards, one batch of compressions per level.

Words are canonical."""
import numpy as np

from tests import _memory_tree_ref as tref

P = tref.P
MALFORMED, WRONG_ROOT = 19, 20


def opening(tree, keys):
    """tree: a SparseTree -> (payloads [n, 8], siblings [m, 8]): for every level, bottom up, and every touched node of it by index, the
    digest of its sibling unless the sibling is touched too"""
    keys = [int(k) for k in keys]
    zero8 = np.zeros(8, np.uint32)
    payloads = np.array([tree.payload.get(k, zero8) for k in keys], np.uint32).reshape(len(keys), 8)
    touched, siblings = set(keys), []
    for level in range(tree.height):
        siblings += [tree.digest(level, t ^ 1) for t in sorted(touched) if (t ^ 1) not in touched]
        touched = {t >> 1 for t in touched}
    return payloads, np.array(siblings, np.uint32).reshape(len(siblings), 8)


def sibling_count(height, keys):
    touched, count = {int(k) for k in keys}, 0
    for _ in range(height):
        count += sum((t ^ 1) not in touched for t in touched)
        touched = {t >> 1 for t in touched}
    return count


def verify(height, root, keys, payloads, siblings, constants):
    """0, MALFORMED or WRONG_ROOT, by the rules of pw_memory_opening_verify"""
    keys = [int(k) for k in keys]
    payloads = np.asarray(payloads, np.uint32).reshape(-1, 8)
    siblings = np.asarray(siblings, np.uint32).reshape(-1, 8)
    root = np.asarray(root, np.uint32).reshape(-1)
    if not 1 <= height <= 40 or not keys or len(payloads) != len(keys) or len(root) != 8:
        return MALFORMED
    if any(k >> height for k in keys) or any(a >= b for a, b in zip(keys, keys[1:])):
        return MALFORMED
    if (root >= P).any() or (payloads >= P).any() or (siblings >= P).any() or len(siblings) != sibling_count(height, keys):
        return MALFORMED
    known = dict(zip(keys, tref.leaf_digests(payloads, constants)))
    rest = list(siblings)
    for _ in range(height):
        parents, pairs = [], []
        for t in sorted(known):
            if t >> 1 in parents[-1:]:
                continue  # the right child of a pair already taken
            other = known[t ^ 1] if (t ^ 1) in known else rest.pop(0)
            pairs.append(np.concatenate([other, known[t]] if t & 1 else [known[t], other]))
            parents.append(t >> 1)
        known = dict(zip(parents, tref.compress(np.array(pairs), constants)))
    assert not rest and list(known) == [0]
    return 0 if (known[0] == root).all() else WRONG_ROOT
