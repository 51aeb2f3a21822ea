/* ================================================================== pw-stark v1: ONE proof per segment ("PWS3")
 * TEST INFRASTRUCTURE (included by stark_oracle.cpp, inside its anonymous namespace). Parity unpinned like the rest of
 * the prover (see the header of stark_oracle.cpp).
 *
 * The reference makes one engine call per segment with the traces of ALL chips, `engine.prove(pk, ProvingContext{
 * per_trace})` (/root/reference/openvm/src/trace_generation.rs:136-139, openvm-riscv/src/lib.rs:327-332), and its
 * backend commits all matrices of a phase together and opens them with one low-degree test. v0 (above) proves one AIR;
 * this is the multi-matrix form, in the shape of Plonky3's mixed-height MMCS + two-adic FRI with reduced openings
 * rolled in by height:
 *
 *   AIRs a = 0..A-1, trace T_a of W_a columns x H_a = 2^(n_a) rows, LDE on the coset s<g_(n_a + 1)> (N_a = 2 H_a points),
 *   N = max N_a = 2^L.
 *
 *   mixed(M_0..M_(A-1)): ONE Merkle tree over matrices of different heights, all in natural order.
 *       level N:   d[j] = H(rows j of the matrices of height N, concatenated in AIR order)         (sponge as v0)
 *       level n<N: d[j] = compress(prev[j], prev[j + n]),  j < n   — siblings are (j, j + n), the pairing of the FRI fold
 *                  if matrices of height n exist:  d[j] = compress(d[j], H(their rows j, concatenated))
 *       root = level 1. Opening at index q: the rows q mod N_a of every matrix + the L siblings prev[(p + n) mod 2n].
 *   transcript: MAGIC3, A, logup, num_queries, pow_bits, then (n_a, W_a, #constraints_a, #interactions_a) per AIR
 *   1. root of mixed(LDE of the main traces)
 *   2. logup: al, bl <- transcript (one pair for the whole segment: no bus seed any more); per AIR the permutation
 *      matrix of v0+LogUp (groups, phi); root of mixed(their LDEs); the cumulative sums S_a (A ext values)
 *   3. alpha <- transcript (shared); per AIR the quotient of v0 / v0+LogUp with its own Z_(H_a), split in 2 chunks x 4
 *      coordinates; root of mixed(the 8-column chunk LDEs)
 *   4. zeta <- transcript (shared); per AIR, in this order (also the order of the gamma powers, one running index over
 *      all AIRs): main at zeta | perm at zeta | quotient at zeta | perm at g_(n_a) zeta
 *   5. gamma <- transcript; per height n the reduced opening vector over the AIRs of that height
 *         ro_n[j] = sum_a [ (sum_k gamma^k (f_k(x_j) - f_k(zeta)))/(x_j - zeta) + (sum_k gamma^k (p_k(x_j) - p_k(g zeta)))/(x_j - g zeta) ],
 *         x_j = s g_n^j
 *   6. FRI over the UNSHIFTED subgroups (a vector on the coset s<g_n> is read as the function y -> V(s y) on <g_n>; its
 *      degree is the same): v_0 = ro_N; round l: commit pairs (v_l[i], v_l[i + N_l/2]) as v0; beta_l <- transcript;
 *         v_(l+1)[i] = (a + b)/2 + beta_l (a - b)/(2 w_l^i)  [+ beta_l^2 ro_(N_l / 2)[i] if AIRs of that height exist]
 *      L - 1 rounds down to 2 (equal) values; final value, proof of work, queries as v0.
 *   query q in [0, N): per phase tree the rows (AIR order) + L siblings; then the FRI layers as v0.
 *   The verifier accepts a segment when the proof verifies and (optionally) sum_a S_a = 0.
 */
constexpr u32 MAGIC3 = 0x33535750u; /* "PWS3" */

struct SegAir {
    const u32* trace; /* column-major W x H, canonical; NULL for the verifier */
    u32 width, log_h;
    Program prog;
    Interactions I;
};

struct MatRef { const u32* m; size_t height, width; };

Digest hash_rows_concat(const std::vector<MatRef>& mats, size_t j) {
    std::vector<u32> row;
    for (const auto& M : mats) for (size_t c = 0; c < M.width; ++c) row.push_back(M.m[c * M.height + j]);
    return hash_row(row.data(), row.size());
}

struct MixedTree {
    std::vector<std::vector<Digest>> levels; /* sizes N, N/2, ..., 1 */
    void build(const std::vector<MatRef>& mats) {
        size_t N = 0;
        for (const auto& M : mats) if (M.height > N) N = M.height;
        levels.clear();
        for (size_t n = N; n >= 1; n >>= 1) {
            std::vector<MatRef> here;
            for (const auto& M : mats) if (M.height == n) here.push_back(M);
            std::vector<Digest> lv(n);
            const std::vector<Digest>* prev = levels.empty() ? nullptr : &levels.back();
#pragma omp parallel for schedule(static)
            for (long j = 0; j < (long)n; ++j) {
                if (!prev) lv[j] = hash_rows_concat(here, (size_t)j);
                else {
                    lv[j] = compress((*prev)[j], (*prev)[j + n]);
                    if (!here.empty()) lv[j] = compress(lv[j], hash_rows_concat(here, (size_t)j));
                }
            }
            levels.push_back(std::move(lv));
        }
    }
    const Digest& root() const { return levels.back()[0]; }
    void path(size_t q, std::vector<u32>& out) const {
        for (size_t l = 0; l + 1 < levels.size(); ++l) {
            const size_t size = levels[l].size(), p = q & (size - 1);
            const Digest& sib = levels[l][(p + size / 2) & (size - 1)];
            out.insert(out.end(), sib.begin(), sib.end());
        }
    }
};

/* per-AIR shape numbers shared by prover and verifier */
struct SegShape {
    size_t H, N; int logN;
    std::vector<u32> gs; size_t n_g, Wp, M, K; /* K = opened polynomials of this AIR */
    size_t koff;                               /* offset of its gamma powers */
};
std::vector<SegShape> seg_shapes(const std::vector<SegAir>& airs, bool logup, size_t& K_total, int& L) {
    std::vector<SegShape> sh(airs.size());
    K_total = 0; L = 0;
    for (size_t a = 0; a < airs.size(); ++a) {
        SegShape& s = sh[a];
        s.H = (size_t)1 << airs[a].log_h; s.N = 2 * s.H; s.logN = (int)airs[a].log_h + 1;
        if (s.logN > L) L = s.logN;
        if (logup) { s.gs = group_starts(airs[a].I); if (s.gs.empty()) s.gs.push_back(0); s.n_g = s.gs.size() - 1; s.Wp = 4 * (s.n_g + 1); }
        else { s.n_g = 0; s.Wp = 0; }
        s.M = airs[a].prog.n + (logup ? s.n_g + 3 : 0);
        s.K = airs[a].width + 2 * s.Wp + 8;
        s.koff = K_total;
        K_total += s.K;
    }
    return sh;
}

void seg_observe_header(Challenger& ch, Writer* pf, const Config& cfg, const std::vector<SegAir>& airs, bool logup) {
    const u32 hdr[5] = {MAGIC3, (u32)airs.size(), logup ? 1u : 0u, cfg.num_queries, cfg.pow_bits};
    for (u32 x : hdr) { ch.observe(x % P); if (pf) pf->put(x); }
    for (const auto& A : airs)
        for (u32 x : {A.log_h, A.width, (u32)A.prog.n, (u32)(logup ? A.I.n : 0)}) { ch.observe(x % P); if (pf) pf->put(x); }
}

std::vector<u32> prove_segment(const Config& cfg, const std::vector<SegAir>& airs, bool logup) {
    const size_t A = airs.size();
    size_t K_total; int L;
    std::vector<SegShape> sh = seg_shapes(airs, logup, K_total, L);
    const size_t Nmax = (size_t)1 << L;
    Writer pf;
    Challenger ch;
    seg_observe_header(ch, &pf, cfg, airs, logup);

    /* 1. main traces */
    std::vector<std::vector<u32>> coef(A), lde(A);
    for (size_t a = 0; a < A; ++a) {
        const size_t H = sh[a].H, N = sh[a].N, W = airs[a].width;
        coef[a].resize(W * H); lde[a].resize(W * N);
#pragma omp parallel for schedule(dynamic)
        for (long c = 0; c < (long)W; ++c) {
            memcpy(&coef[a][c * H], airs[a].trace + c * H, H * 4);
            idft(&coef[a][c * H], (int)airs[a].log_h);
            coset_lde_from_coeffs(&coef[a][c * H], (int)airs[a].log_h, &lde[a][c * N]);
        }
    }
    MixedTree t_tree;
    { std::vector<MatRef> m; for (size_t a = 0; a < A; ++a) m.push_back({lde[a].data(), sh[a].N, airs[a].width}); t_tree.build(m); }
    pf.put(t_tree.root());
    ch.observe_digest(t_tree.root());

    /* 2. LogUp */
    Ext al = ext_zero(), bl = ext_zero();
    std::vector<std::vector<Ext>> blpow(A);
    std::vector<std::vector<u32>> perm(A), pcoef(A), plde(A);
    std::vector<Ext> S(A, ext_zero());
    auto group_fraction = [&](size_t a, size_t g, const u32* m, size_t stride, size_t row, Ext& num, Ext& den) {
        num = ext_zero(); den = ext_one();
        for (size_t i = sh[a].gs[g]; i < sh[a].gs[g + 1]; ++i) {
            Ext d = LogupRow::denom_base(airs[a].I, i, m, stride, row, al, blpow[a].data());
            u32 mu = LogupRow::mult_base(airs[a].I, i, m, stride, row);
            num = ext_add(ext_mul(num, d), ext_scale(den, mu));
            den = ext_mul(den, d);
        }
    };
    MixedTree p_tree;
    if (logup) {
        al = ch.sample_ext();
        bl = ch.sample_ext();
        for (size_t a = 0; a < A; ++a) {
            const size_t H = sh[a].H, N = sh[a].N, n_g = sh[a].n_g, Wp = sh[a].Wp;
            blpow[a].resize(max_args(airs[a].I) + 2);
            { Ext b = ext_one(); for (auto& x : blpow[a]) { x = b; b = ext_mul(b, bl); } }
            perm[a].assign(Wp * H, 0);
            std::vector<Ext> rowsum(H);
#pragma omp parallel for schedule(static)
            for (long r = 0; r < (long)H; ++r) {
                Ext acc = ext_zero();
                for (size_t g = 0; g < n_g; ++g) {
                    Ext num, den;
                    group_fraction(a, g, airs[a].trace, H, (size_t)r, num, den);
                    Ext q = ext_mul(num, ext_inv(den));
                    for (int k = 0; k < 4; ++k) perm[a][(4 * g + k) * H + r] = q.c[k];
                    acc = ext_add(acc, q);
                }
                rowsum[r] = acc;
            }
            Ext run = ext_zero();
            for (size_t r = 0; r < H; ++r) { run = ext_add(run, rowsum[r]); for (int k = 0; k < 4; ++k) perm[a][(4 * n_g + k) * H + r] = run.c[k]; }
            S[a] = run;
            pcoef[a].resize(Wp * H); plde[a].resize(Wp * N);
#pragma omp parallel for schedule(dynamic)
            for (long c = 0; c < (long)Wp; ++c) {
                memcpy(&pcoef[a][c * H], &perm[a][c * H], H * 4);
                idft(&pcoef[a][c * H], (int)airs[a].log_h);
                coset_lde_from_coeffs(&pcoef[a][c * H], (int)airs[a].log_h, &plde[a][c * N]);
            }
        }
        { std::vector<MatRef> m; for (size_t a = 0; a < A; ++a) m.push_back({plde[a].data(), sh[a].N, sh[a].Wp}); p_tree.build(m); }
        pf.put(p_tree.root());
        ch.observe_digest(p_tree.root());
        for (size_t a = 0; a < A; ++a) { pf.put(S[a]); ch.observe_ext(S[a]); }
    }

    /* 3. quotients */
    const Ext alpha = ch.sample_ext();
    std::vector<std::vector<u32>> qcoef(A), qlde(A);
    for (size_t a = 0; a < A; ++a) {
        const size_t H = sh[a].H, N = sh[a].N, n_g = sh[a].n_g, M = sh[a].M, nc = airs[a].prog.n;
        const int logN = sh[a].logN;
        const Program& prog = airs[a].prog;
        std::vector<Ext> apow(M ? M : 1);
        { Ext x = ext_one(); for (size_t j = M; j-- > 0;) { apow[j] = x; x = ext_mul(x, alpha); } }
        const u32 sH = or_pow(COSET_SHIFT, H);
        const u32 zval[2] = {or_sub(sH, 1), or_sub(or_neg(sH), 1)};
        const u32 zinv[2] = {or_inv(zval[0]), or_inv(zval[1])};
        const u32 ginv = or_inv(root_of_unity((int)airs[a].log_h));
        const u32 wN = root_of_unity(logN);
        std::vector<u32> xs(N);
        { u32 x = COSET_SHIFT; for (size_t j = 0; j < N; ++j) { xs[j] = x; x = or_mul(x, wN); } }
        std::vector<u32> q(4 * N);
#pragma omp parallel for schedule(static)
        for (long j = 0; j < (long)N; ++j) {
            Ext acc = ext_zero();
            for (size_t k = 0; k < nc; ++k) {
                u32 v = eval_base(prog.bc + prog.spans[2 * k], prog.spans[2 * k + 1], lde[a].data(), N, (size_t)j);
                acc = ext_add(acc, ext_scale(apow[k], v));
            }
            if (logup) {
                const size_t jn = ((size_t)j + 2) & (N - 1);
                Ext sumq = ext_zero(), sumq_next = ext_zero();
                for (size_t g = 0; g < n_g; ++g) {
                    Ext qi, qn, num, den;
                    for (int k = 0; k < 4; ++k) { qi.c[k] = plde[a][(4 * g + k) * N + j]; qn.c[k] = plde[a][(4 * g + k) * N + jn]; }
                    sumq = ext_add(sumq, qi);
                    sumq_next = ext_add(sumq_next, qn);
                    group_fraction(a, g, lde[a].data(), N, (size_t)j, num, den);
                    acc = ext_add(acc, ext_mul(apow[nc + g], ext_sub(ext_mul(qi, den), num)));
                }
                Ext phi, phin;
                for (int k = 0; k < 4; ++k) { phi.c[k] = plde[a][(4 * n_g + k) * N + j]; phin.c[k] = plde[a][(4 * n_g + k) * N + jn]; }
                const u32 x = xs[j], Z = zval[j & 1];
                const u32 is_first = or_mul(Z, or_inv(or_sub(x, 1)));
                const u32 is_last = or_mul(Z, or_inv(or_sub(x, ginv)));
                const u32 is_trans = or_sub(x, ginv);
                acc = ext_add(acc, ext_mul(apow[nc + n_g], ext_scale(ext_sub(phi, sumq), is_first)));
                acc = ext_add(acc, ext_mul(apow[nc + n_g + 1], ext_scale(ext_sub(ext_sub(phin, phi), sumq_next), is_trans)));
                acc = ext_add(acc, ext_mul(apow[nc + n_g + 2], ext_scale(ext_sub(phi, S[a]), is_last)));
            }
            acc = ext_scale(acc, zinv[j & 1]);
            for (int k = 0; k < 4; ++k) q[k * N + j] = acc.c[k];
        }
        qcoef[a].resize(8 * H); qlde[a].resize(8 * N);
        const u32 sinv = or_inv(COSET_SHIFT);
        for (int k = 0; k < 4; ++k) {
            idft(&q[k * N], logN);
            u32 sp = 1;
            for (size_t i = 0; i < N; ++i) { q[k * N + i] = or_mul(q[k * N + i], sp); sp = or_mul(sp, sinv); }
            memcpy(&qcoef[a][(size_t)k * H], &q[k * N], H * 4);
            memcpy(&qcoef[a][(size_t)(4 + k) * H], &q[k * N + H], H * 4);
        }
        for (int c = 0; c < 8; ++c) coset_lde_from_coeffs(&qcoef[a][(size_t)c * H], (int)airs[a].log_h, &qlde[a][(size_t)c * N]);
    }
    MixedTree q_tree;
    { std::vector<MatRef> m; for (size_t a = 0; a < A; ++a) m.push_back({qlde[a].data(), sh[a].N, 8}); q_tree.build(m); }
    pf.put(q_tree.root());
    ch.observe_digest(q_tree.root());

    /* 4. openings: per AIR main | perm@zeta | quotient | perm@g zeta */
    const Ext zeta = ch.sample_ext();
    std::vector<Ext> opened(K_total);
    std::vector<Ext> gzeta(A);
    for (size_t a = 0; a < A; ++a) {
        const size_t H = sh[a].H, W = airs[a].width, Wp = sh[a].Wp;
        gzeta[a] = ext_scale(zeta, root_of_unity((int)airs[a].log_h));
        Ext* o = &opened[sh[a].koff];
#pragma omp parallel for schedule(dynamic)
        for (long c = 0; c < (long)W; ++c) o[c] = eval_poly_at(&coef[a][c * H], H, zeta);
#pragma omp parallel for schedule(dynamic)
        for (long c = 0; c < (long)Wp; ++c) {
            o[W + c] = eval_poly_at(&pcoef[a][c * H], H, zeta);
            o[W + Wp + 8 + c] = eval_poly_at(&pcoef[a][c * H], H, gzeta[a]);
        }
        for (int c = 0; c < 8; ++c) o[W + Wp + c] = eval_poly_at(&qcoef[a][(size_t)c * H], H, zeta);
    }
    for (const Ext& e : opened) { pf.put(e); ch.observe_ext(e); }

    /* 5. reduced openings per height */
    const Ext gamma = ch.sample_ext();
    std::vector<Ext> gpow(K_total);
    { Ext g = ext_one(); for (size_t k = 0; k < K_total; ++k) { gpow[k] = g; g = ext_mul(g, gamma); } }
    std::vector<std::vector<Ext>> ro(L + 1); /* ro[log n] */
    for (size_t a = 0; a < A; ++a) {
        const size_t N = sh[a].N, W = airs[a].width, Wp = sh[a].Wp, K1 = W + Wp + 8;
        const Ext* gp = &gpow[sh[a].koff];
        const Ext* o = &opened[sh[a].koff];
        Ext sum1 = ext_zero(), sum2 = ext_zero();
        for (size_t k = 0; k < K1; ++k) sum1 = ext_add(sum1, ext_mul(gp[k], o[k]));
        for (size_t k = K1; k < K1 + Wp; ++k) sum2 = ext_add(sum2, ext_mul(gp[k], o[k]));
        std::vector<Ext>& v = ro[sh[a].logN];
        if (v.empty()) v.assign(N, ext_zero());
        const u32 wN = root_of_unity(sh[a].logN);
        std::vector<u32> xs(N);
        { u32 x = COSET_SHIFT; for (size_t j = 0; j < N; ++j) { xs[j] = x; x = or_mul(x, wN); } }
#pragma omp parallel for schedule(static)
        for (long j = 0; j < (long)N; ++j) {
            Ext a1 = ext_zero(), a2 = ext_zero();
            for (size_t k = 0; k < W; ++k) a1 = ext_add(a1, ext_scale(gp[k], lde[a][k * N + j]));
            for (size_t k = 0; k < Wp; ++k) {
                const u32 pv = plde[a][k * N + j];
                a1 = ext_add(a1, ext_scale(gp[W + k], pv));
                a2 = ext_add(a2, ext_scale(gp[K1 + k], pv));
            }
            for (size_t k = 0; k < 8; ++k) a1 = ext_add(a1, ext_scale(gp[W + Wp + k], qlde[a][k * N + j]));
            Ext t = ext_mul(ext_sub(a1, sum1), ext_inv(ext_sub(ext_from(xs[j]), zeta)));
            if (logup) t = ext_add(t, ext_mul(ext_sub(a2, sum2), ext_inv(ext_sub(ext_from(xs[j]), gzeta[a]))));
            v[j] = ext_add(v[j], t);
        }
    }

    /* 6. FRI on the unshifted subgroups, reduced openings of smaller heights rolled in */
    std::vector<std::vector<Ext>> layers;
    std::vector<Merkle> fri_trees;
    std::vector<Ext> v = ro[L];
    const u32 inv2 = or_inv(2);
    for (int l = 0; l + 1 < L; ++l) {
        const size_t Nl = Nmax >> l, half = Nl / 2;
        std::vector<Digest> leaves(half);
#pragma omp parallel for schedule(static)
        for (long i = 0; i < (long)half; ++i) {
            u32 row[8];
            memcpy(row, v[i].c, 16);
            memcpy(row + 4, v[i + half].c, 16);
            leaves[i] = hash_row(row, 8);
        }
        Merkle t;
        t.build(std::move(leaves));
        pf.put(t.root());
        ch.observe_digest(t.root());
        const Ext beta = ch.sample_ext();
        const Ext beta2 = ext_mul(beta, beta);
        const u32 wl = root_of_unity(L - l);
        std::vector<u32> xl(half);
        { u32 x = 1; for (size_t i = 0; i < half; ++i) { xl[i] = x; x = or_mul(x, wl); } }
        const std::vector<Ext>& roll = ro[L - l - 1];
        std::vector<Ext> nv(half);
#pragma omp parallel for schedule(static)
        for (long i = 0; i < (long)half; ++i) {
            Ext x0 = v[i], x1 = v[i + half];
            Ext s2 = ext_scale(ext_add(x0, x1), inv2);
            Ext d = ext_scale(ext_sub(x0, x1), or_mul(inv2, or_inv(xl[i])));
            nv[i] = ext_add(s2, ext_mul(beta, d));
            if (!roll.empty()) nv[i] = ext_add(nv[i], ext_mul(beta2, roll[i]));
        }
        layers.push_back(std::move(v));
        fri_trees.push_back(std::move(t));
        v = std::move(nv);
    }
    pf.put(v[0]);
    ch.observe_ext(v[0]);
    u32 witness = 0;
    if (cfg.pow_bits) {
        for (;; ++witness) { Challenger c2 = ch; c2.observe(witness); if (c2.sample_bits((int)cfg.pow_bits) == 0) break; }
    }
    pf.put(witness);
    ch.observe(witness);
    if (cfg.pow_bits) (void)ch.sample_bits((int)cfg.pow_bits);

    /* 7. queries */
    for (u32 qi = 0; qi < cfg.num_queries; ++qi) {
        const size_t q = ch.sample_bits(L);
        pf.put((u32)q);
        for (size_t a = 0; a < A; ++a) { const size_t N = sh[a].N, r = q & (N - 1); for (size_t c = 0; c < airs[a].width; ++c) pf.put(lde[a][c * N + r]); }
        t_tree.path(q, pf.w);
        if (logup) {
            for (size_t a = 0; a < A; ++a) { const size_t N = sh[a].N, r = q & (N - 1); for (size_t c = 0; c < sh[a].Wp; ++c) pf.put(plde[a][c * N + r]); }
            p_tree.path(q, pf.w);
        }
        for (size_t a = 0; a < A; ++a) { const size_t N = sh[a].N, r = q & (N - 1); for (size_t c = 0; c < 8; ++c) pf.put(qlde[a][c * N + r]); }
        q_tree.path(q, pf.w);
        for (int l = 0; l + 1 < L; ++l) {
            const size_t Nl = Nmax >> l, half = Nl / 2, p = q & (Nl - 1);
            pf.put(layers[l][p ^ half]);
            fri_trees[l].path(p & (half - 1), pf.w);
        }
    }
    return pf.w;
}

/* 0 = valid; codes as verify()/verify_logup() plus 14 = the cumulative bus sums do not cancel (check_balance),
 * 15 = malformed segment description (or_verify_segment also answers it for a malformed PROGRAM of an AIR, before this is called:
 * `validation` in stark_oracle.cpp). total_sum4 (may be NULL) receives sum_a S_a. */
int verify_segment(const Config& cfg, const u32* proof, size_t len, const std::vector<SegAir>& airs, bool logup, bool check_balance,
                   u32* total_sum4) {
    const size_t A = airs.size();
    if (!A) return 15;
    for (const auto& a : airs) if (a.log_h < 1 || a.log_h > 26 || !a.width) return 15;
    size_t K_total; int L;
    std::vector<SegShape> sh = seg_shapes(airs, logup, K_total, L);
    const size_t Nmax = (size_t)1 << L;
    size_t pos = 0;
    auto need = [&](size_t k) { if (pos + k > len) throw std::runtime_error("short proof"); };
    auto get = [&]() { need(1); return proof[pos++]; };
    auto get_digest = [&]() { need(8); Digest d; memcpy(d.data(), proof + pos, 32); pos += 8; return d; };
    auto get_ext = [&]() { need(4); Ext e; memcpy(e.c, proof + pos, 16); pos += 4; return e; };
    try {
        Challenger ch;
        {
            Writer hdr;
            seg_observe_header(ch, &hdr, cfg, airs, logup);
            need(hdr.w.size());
            if (memcmp(hdr.w.data(), proof, hdr.w.size() * 4) != 0) return 1;
            pos = hdr.w.size();
        }
        for (size_t i = 0; i < len; ++i) if (proof[i] >= P) return 13;
        const Digest t_root = get_digest();
        ch.observe_digest(t_root);
        Ext al = ext_zero(), bl = ext_zero();
        Digest p_root{};
        std::vector<Ext> S(A, ext_zero());
        if (logup) {
            al = ch.sample_ext();
            bl = ch.sample_ext();
            p_root = get_digest();
            ch.observe_digest(p_root);
            for (size_t a = 0; a < A; ++a) { S[a] = get_ext(); ch.observe_ext(S[a]); }
        }
        const Ext alpha = ch.sample_ext();
        const Digest q_root = get_digest();
        ch.observe_digest(q_root);
        const Ext zeta = ch.sample_ext();
        std::vector<Ext> opened(K_total);
        for (auto& e : opened) { e = get_ext(); ch.observe_ext(e); }
        /* constraint identities at zeta, AIR by AIR */
        const Ext basis[4] = {{{1, 0, 0, 0}}, {{0, 1, 0, 0}}, {{0, 0, 1, 0}}, {{0, 0, 0, 1}}};
        std::vector<Ext> gzeta(A);
        for (size_t a = 0; a < A; ++a) {
            const size_t W = airs[a].width, Wp = sh[a].Wp, n_g = sh[a].n_g, H = sh[a].H;
            const Ext* o = &opened[sh[a].koff];
            const Program& prog = airs[a].prog;
            const Interactions& I = airs[a].I;
            const u32 g = root_of_unity((int)airs[a].log_h), ginv = or_inv(g);
            gzeta[a] = ext_scale(zeta, g);
            auto ext_col = [&](size_t base) { Ext r = ext_zero(); for (int k = 0; k < 4; ++k) r = ext_add(r, ext_mul(basis[k], o[base + k])); return r; };
            Ext acc = ext_zero();
            for (size_t k = 0; k < prog.n; ++k) acc = ext_add(ext_mul(acc, alpha), eval_ext(prog.bc + prog.spans[2 * k], prog.spans[2 * k + 1], o));
            const Ext zH = ext_pow(zeta, H);
            const Ext Z = ext_sub(zH, ext_one());
            if (logup) {
                std::vector<Ext> blpow(max_args(I) + 2);
                { Ext b = ext_one(); for (auto& x : blpow) { x = b; b = ext_mul(b, bl); } }
                const size_t K1 = W + Wp + 8;
                Ext sumq = ext_zero(), sumq_next = ext_zero();
                for (size_t gi = 0; gi < n_g; ++gi) {
                    Ext num = ext_zero(), den = ext_one();
                    for (size_t i = sh[a].gs[gi]; i < sh[a].gs[gi + 1]; ++i) {
                        const u32* it = I.inter + 3 * i;
                        const u32* sp = I.spans + 2 * (size_t)it[2];
                        Ext d = ext_add(al, ext_from(it[0] % P));
                        for (u32 j = 0; j < it[1]; ++j) d = ext_add(d, ext_mul(blpow[j + 1], eval_ext(I.bc + sp[2 + 2 * j], sp[3 + 2 * j], o)));
                        Ext m = eval_ext(I.bc + sp[0], sp[1], o);
                        num = ext_add(ext_mul(num, d), ext_mul(den, m));
                        den = ext_mul(den, d);
                    }
                    Ext qi = ext_col(W + 4 * gi), qn = ext_col(K1 + 4 * gi);
                    sumq = ext_add(sumq, qi);
                    sumq_next = ext_add(sumq_next, qn);
                    acc = ext_add(ext_mul(acc, alpha), ext_sub(ext_mul(qi, den), num));
                }
                Ext phi = ext_col(W + 4 * n_g), phin = ext_col(K1 + 4 * n_g);
                Ext is_first = ext_mul(Z, ext_inv(ext_sub(zeta, ext_one())));
                Ext is_last = ext_mul(Z, ext_inv(ext_sub(zeta, ext_from(ginv))));
                Ext is_trans = ext_sub(zeta, ext_from(ginv));
                acc = ext_add(ext_mul(acc, alpha), ext_mul(is_first, ext_sub(phi, sumq)));
                acc = ext_add(ext_mul(acc, alpha), ext_mul(is_trans, ext_sub(ext_sub(phin, phi), sumq_next)));
                acc = ext_add(ext_mul(acc, alpha), ext_mul(is_last, ext_sub(phi, S[a])));
            }
            Ext qlo = ext_col(W + Wp), qhi = ext_col(W + Wp + 4);
            if (!ext_eq(acc, ext_mul(Z, ext_add(qlo, ext_mul(zH, qhi))))) return (int)((a + 1) << 8) | 2;
        }
        const Ext gamma = ch.sample_ext();
        std::vector<Ext> gpow(K_total);
        { Ext g = ext_one(); for (size_t k = 0; k < K_total; ++k) { gpow[k] = g; g = ext_mul(g, gamma); } }
        std::vector<Ext> sum1(A, ext_zero()), sum2(A, ext_zero());
        for (size_t a = 0; a < A; ++a) {
            const size_t K1 = airs[a].width + sh[a].Wp + 8;
            for (size_t k = 0; k < K1; ++k) sum1[a] = ext_add(sum1[a], ext_mul(gpow[sh[a].koff + k], opened[sh[a].koff + k]));
            for (size_t k = K1; k < sh[a].K; ++k) sum2[a] = ext_add(sum2[a], ext_mul(gpow[sh[a].koff + k], opened[sh[a].koff + k]));
        }
        const int rounds = L - 1;
        std::vector<Digest> fri_roots(rounds);
        std::vector<Ext> betas(rounds);
        for (int l = 0; l < rounds; ++l) { fri_roots[l] = get_digest(); ch.observe_digest(fri_roots[l]); betas[l] = ch.sample_ext(); }
        const Ext final_poly = get_ext();
        ch.observe_ext(final_poly);
        const u32 witness = get();
        ch.observe(witness);
        if (cfg.pow_bits && ch.sample_bits((int)cfg.pow_bits) != 0) return 3;

        /* opening of a mixed tree: rows[a] = pointer to AIR a's row in the proof, widths[a] */
        auto check_mixed = [&](const std::vector<const u32*>& rows, const std::vector<size_t>& widths, size_t q, const Digest& root) {
            auto hash_level = [&](size_t n, bool& any) {
                std::vector<u32> row;
                any = false;
                for (size_t a = 0; a < A; ++a) if (sh[a].N == n) { any = true; row.insert(row.end(), rows[a], rows[a] + widths[a]); }
                return hash_row(row.data(), row.size());
            };
            bool any;
            Digest cur = hash_level(Nmax, any);
            size_t p = q;
            for (size_t n = Nmax / 2; n >= 1; n >>= 1) {
                Digest sib = get_digest();
                cur = (p & n) ? compress(sib, cur) : compress(cur, sib);
                p &= n - 1;
                Digest inj = hash_level(n, any);
                if (any) cur = compress(cur, inj);
            }
            return cur == root;
        };
        auto check_path = [&](Digest leaf, size_t idx, int depth, const Digest& root) {
            for (int l = 0; l < depth; ++l) { Digest sib = get_digest(); leaf = ((idx >> l) & 1) ? compress(sib, leaf) : compress(leaf, sib); }
            return leaf == root;
        };
        const u32 inv2 = or_inv(2);
        std::vector<const u32*> trow(A), prow(A), qrow(A);
        std::vector<size_t> wt(A), wp(A), wq(A, 8);
        for (size_t a = 0; a < A; ++a) { wt[a] = airs[a].width; wp[a] = sh[a].Wp; }
        for (u32 qi = 0; qi < cfg.num_queries; ++qi) {
            const size_t q = ch.sample_bits(L);
            if (get() != q) return 4;
            for (size_t a = 0; a < A; ++a) { need(wt[a]); trow[a] = proof + pos; pos += wt[a]; }
            if (!check_mixed(trow, wt, q, t_root)) return 5;
            if (logup) {
                for (size_t a = 0; a < A; ++a) { need(wp[a]); prow[a] = proof + pos; pos += wp[a]; }
                if (!check_mixed(prow, wp, q, p_root)) return 11;
            }
            for (size_t a = 0; a < A; ++a) { need(8); qrow[a] = proof + pos; pos += 8; }
            if (!check_mixed(qrow, wq, q, q_root)) return 6;
            /* reduced opening of height 2^logn at index q mod 2^logn */
            auto ro_at = [&](int logn, bool& any) {
                Ext r = ext_zero();
                any = false;
                const size_t n = (size_t)1 << logn;
                for (size_t a = 0; a < A; ++a) {
                    if (sh[a].logN != logn) continue;
                    any = true;
                    const size_t W = wt[a], Wp = wp[a], K1 = W + Wp + 8;
                    const Ext* gp = &gpow[sh[a].koff];
                    const u32 x = or_mul(COSET_SHIFT, or_pow(root_of_unity(logn), q & (n - 1)));
                    Ext a1 = ext_zero(), a2 = ext_zero();
                    for (size_t k = 0; k < W; ++k) a1 = ext_add(a1, ext_scale(gp[k], trow[a][k]));
                    for (size_t k = 0; k < Wp; ++k) { a1 = ext_add(a1, ext_scale(gp[W + k], prow[a][k])); a2 = ext_add(a2, ext_scale(gp[K1 + k], prow[a][k])); }
                    for (size_t k = 0; k < 8; ++k) a1 = ext_add(a1, ext_scale(gp[W + Wp + k], qrow[a][k]));
                    Ext t = ext_mul(ext_sub(a1, sum1[a]), ext_inv(ext_sub(ext_from(x), zeta)));
                    if (logup) t = ext_add(t, ext_mul(ext_sub(a2, sum2[a]), ext_inv(ext_sub(ext_from(x), gzeta[a]))));
                    r = ext_add(r, t);
                }
                return r;
            };
            bool any;
            Ext cur = ro_at(L, any);
            for (int l = 0; l < rounds; ++l) {
                const size_t Nl = Nmax >> l, half = Nl / 2, p = q & (Nl - 1);
                const Ext sib = get_ext();
                const Ext lo = (p < half) ? cur : sib, hi = (p < half) ? sib : cur;
                u32 row[8];
                memcpy(row, lo.c, 16); memcpy(row + 4, hi.c, 16);
                if (!check_path(hash_row(row, 8), p & (half - 1), L - 1 - l, fri_roots[l])) return 7;
                const u32 xi = or_pow(root_of_unity(L - l), p & (half - 1));
                Ext s2 = ext_scale(ext_add(lo, hi), inv2);
                Ext d = ext_scale(ext_sub(lo, hi), or_mul(inv2, or_inv(xi)));
                cur = ext_add(s2, ext_mul(betas[l], d));
                Ext roll = ro_at(L - l - 1, any);
                if (any) cur = ext_add(cur, ext_mul(ext_mul(betas[l], betas[l]), roll));
            }
            if (!ext_eq(cur, final_poly)) return 8;
        }
        if (pos != len) return 9;
        Ext total = ext_zero();
        for (size_t a = 0; a < A; ++a) total = ext_add(total, S[a]);
        if (total_sum4) memcpy(total_sum4, total.c, 16);
        if (logup && check_balance && !ext_eq(total, ext_zero())) return 14;
    } catch (const std::exception&) {
        return 10;
    }
    return 0;
}
