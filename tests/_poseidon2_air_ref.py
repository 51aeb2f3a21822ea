"""The numpy reference of the Poseidon2 compression chip (powdr_amd/system_airs.py poseidon2_air, pw_poseidon2_compress_trace; DESIGN.md
§5l): the permutation restated with plain `% p` arithmetic on canonical words, returning every intermediate the AIR commits, and the
trace the device generator must write for a list of requests.

Layout (307 columns): mult | in[16] | per full round r = 0..7: cube[r][16], sbox[r][16] | per partial round k = 0..12: pcube[k],
psbox[k] | out[8]. Constants: (ext_rc[8][16], int_rc[13], diag[16]) canonical, as prover.poseidon2_constants() returns them."""
import numpy as np

P = 0x78000001
WIDTH = 307
IN, FULL, PARTIAL, OUT = 1, 17, 273, 299
M4 = np.array([[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]], np.int64)


def external_layer(s):
    """s: [16, n] int64 -> M4 on each block of four words, then every word gets the sum of its column over the four blocks"""
    t = np.concatenate([M4 @ s[4 * b:4 * b + 4] % P for b in range(4)])
    col = sum(t[4 * b:4 * b + 4] for b in range(4)) % P
    return (t + np.tile(col, (4, 1))) % P


def permute(inputs, constants):
    """inputs: [n, 16] canonical words -> (final state [n, 16], trace cells [307, n] with mult = 0)"""
    ext_rc, int_rc, diag = (np.asarray(c).astype(np.int64) for c in constants)
    s = np.ascontiguousarray(np.asarray(inputs, dtype=np.int64).reshape(-1, 16).T)
    n = s.shape[1]
    cells = np.zeros((WIDTH, n), np.int64)
    cells[IN:IN + 16] = s

    def full(r, s):
        x = (s + ext_rc[r][:, None]) % P
        cube = x * x % P * x % P
        sbox = cube * cube % P * x % P
        cells[FULL + 32 * r:FULL + 32 * r + 16] = cube
        cells[FULL + 32 * r + 16:FULL + 32 * r + 32] = sbox
        return external_layer(sbox)

    s = external_layer(s)
    for r in range(4):
        s = full(r, s)
    for k in range(13):
        x = (s[0] + int_rc[k]) % P
        cube = x * x % P * x % P
        s[0] = cube * cube % P * x % P
        cells[PARTIAL + 2 * k], cells[PARTIAL + 2 * k + 1] = cube, s[0]
        s = (s.sum(axis=0) % P + diag[:, None] * s) % P
    for r in range(4, 8):
        s = full(r, s)
    cells[OUT:OUT + 8] = s[:8]
    return s.T.astype(np.uint32), cells


def compress_rows(requests, constants, log_height=None):
    """requests: [(16 input words, centred multiplicity)] in WITNESS ORDER (the order of (air, interaction, row) in which the senders
    are walked). -> (trace [307, 2^log_height] canonical, distinct keys): one row per distinct key in the order of its first witness,
    mult = the sum mod p (a key whose multiplicities cancel keeps its row), padding = the row of the zero input with mult = 0;
    log_height = ceil(log2 keys), at least 1, unless given."""
    keys, mult = {}, []
    for words, m in requests:
        k = tuple(int(w) for w in words)
        if k not in keys:
            keys[k] = len(mult)
            mult.append(0)
        mult[keys[k]] = (mult[keys[k]] + int(m)) % P
    n = len(keys)
    lh = 1
    while (1 << lh) < n:
        lh += 1
    if log_height is not None:
        assert log_height >= lh
        lh = log_height
    inputs = np.zeros((1 << lh, 16), np.int64)
    if n:
        inputs[:n] = np.array(list(keys), np.int64)
    _, cells = permute(inputs, constants)
    cells[0, :n] = mult
    return cells.astype(np.uint32), n


# ---- a hash user: the sender the tests put on the bus ---------------------------------------------------------------------------------
USER_WIDTH = 25  # is_valid, left[8], right[8], out[8]


def hash_user_interactions(bus, n_args=24, range_bus=None):
    """one send of is_valid x (left, right, out) — (interactions, spans, bytecode) as prover.Prover takes them; n_args < 24 drops the
    last words (a malformed sender); range_bus: a second interaction, the range check (left[0], 17) on that bus, is_valid times"""
    inter, spans, bc = [[bus, n_args, 0]], [], []
    for c in range(1 + n_args):
        spans.append((len(bc), 2))
        bc += [0, c]
    if range_bus is not None:
        inter.append([range_bus, 2, len(spans)])
        for code in ([0, 0], [0, 1], [1, 17]):
            spans.append((len(bc), 2))
            bc += code
    return np.array(inter, np.uint32), np.array(spans, np.uint32), np.array(bc, np.uint32)


def hash_user_trace(inputs, constants, log_height, valid=None):
    """[25, 2^log_height] canonical: row r asks for the compression of inputs[r] with the right digest; is_valid = valid[r] (default 1:
    any field element is a multiplicity), rows past the inputs are zero"""
    inputs = np.asarray(inputs, dtype=np.int64).reshape(-1, 16)
    n = len(inputs)
    t = np.zeros((USER_WIDTH, 1 << log_height), np.int64)
    assert n <= t.shape[1]
    t[0, :n] = 1 if valid is None else np.asarray(valid, dtype=np.int64) % P
    t[1:17, :n] = inputs.T
    t[17:25, :n] = permute(inputs, constants)[0].T[:8]
    return t.astype(np.uint32)


def requests_of(host, bus):
    """the requests of a list of sender AIRs [(cols, interactions)] on `bus` in witness order (air, interaction, row): [(16 input
    words, centred multiplicity)] — the interactions' plain-column programs read directly"""
    out = []
    for cols, (inter, spans, bc) in host:
        for b, n_args, first in np.asarray(inter).tolist():
            if b != bus:
                continue
            col = [int(bc[int(spans[first + k][0]) + 1]) for k in range(17)]
            assert all(int(spans[first + k][1]) == 2 and int(bc[int(spans[first + k][0])]) == 0 for k in range(17))
            for r in np.nonzero(cols[col[0]])[0].tolist():
                m = int(cols[col[0]][r])
                out.append(([int(cols[c][r]) for c in col[1:]], m - P if m > P // 2 else m))
    return out
