"""TEST INFRASTRUCTURE — the second route to the superblock statistics, written from the definition: a sequential walk
over the pcs, dictionaries, Python list slicing. No sorting by keys, no fingerprints, no level-by-level names."""


class Status(Exception):
    def __init__(self, status, info):
        super().__init__(f"status {status}, info {info}")
        self.status, self.info = status, info


def find_non_overlapping(haystack, needle):
    """leftmost-greedy: on a match advance by len(needle), otherwise by 1"""
    haystack, needle = list(haystack), list(needle)
    out, pos = [], 0
    while pos + len(needle) <= len(haystack):
        if haystack[pos:pos + len(needle)] == needle:
            out.append(pos)
            pos += len(needle)
        else:
            pos += 1
    return out


def heads(pcs, blocks, pc_step=4, keys=None):
    """the start pcs of the blocks the walk enters, in order; Status(3, the first offending position — or keys[position])"""
    start_of = {int(s): int(n) for s, n in blocks}
    name = (lambda p: p) if keys is None else (lambda p: keys[p])
    out, p = [], 0
    while p < len(pcs):
        s = pcs[p]
        if s not in start_of:
            raise Status(3, name(p))
        n = start_of[s]
        for k in range(1, n):
            if p + k < len(pcs) and pcs[p + k] != s + k * pc_step:
                raise Status(3, name(p + k))
        out.append(s)
        p += n
    return out, start_of


def run_instances(pcs, blocks, pc_step=4, keys=None):
    """every run instance in execution order: the stretches of multi-instruction heads between one-instruction heads"""
    hs, start_of = heads(pcs, blocks, pc_step, keys)
    runs, cur = [], []
    for s in hs:
        if start_of[s] == 1:
            if cur:
                runs.append(cur)
            cur = []
        else:
            cur.append(s)
    if cur:
        runs.append(cur)
    return runs


def superblocks_of(runs, max_bb):
    """{window: the sum over all run instances of its greedy non-overlapping occurrences}"""
    windows = set()
    for run in runs:
        for L in range(1, min(max_bb, len(run)) + 1):
            for i in range(len(run) - L + 1):
                windows.add(tuple(run[i:i + L]))
    distinct = {}
    for run in runs:
        distinct[tuple(run)] = distinct.get(tuple(run), 0) + 1
    counts = {}
    for w in windows:
        counts[w] = sum(len(find_non_overlapping(run, w)) * times for run, times in distinct.items())
    return counts


def detect(pcs, blocks, max_bb=1, pc_step=4, keys=None):
    """dict(pc_count, execution_bb_runs [(run, count)] and superblock_counts {window: count}, both in map order, runs = the instances)"""
    pcs = [int(x) for x in pcs]
    runs = run_instances(pcs, blocks, pc_step, keys)
    pc_count = {}
    for pc in pcs:
        pc_count[pc] = pc_count.get(pc, 0) + 1
    distinct = {}
    for run in runs:
        distinct[tuple(run)] = distinct.get(tuple(run), 0) + 1
    counts = superblocks_of(runs, max_bb)
    return dict(pc_count=dict(sorted(pc_count.items())), execution_bb_runs=sorted(distinct.items()), superblock_counts=dict(sorted(counts.items())), runs=runs)


def count_and_update_run(needle, run):
    """(occurrences, what is left of the run: the non-empty stretches between the matches)"""
    needle, run = list(needle), list(run)
    matches = find_non_overlapping(run, needle)
    edges = [0] + [e for i in matches for e in (i, i + len(needle))] + [len(run)]
    return len(matches), [run[a:b] for a, b in zip(edges[::2], edges[1::2]) if a != b]


def count_and_update_execution(needle, runs):
    """over run instances: (total, the instances afterwards)"""
    total, after = 0, []
    for run in runs:
        n, subs = count_and_update_run(needle, run)
        total += n
        after += subs
    return total, after


def count(needle, runs):
    return sum(len(find_non_overlapping(run, needle)) for run in runs)
