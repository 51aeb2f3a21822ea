// Every byte figure of a segment proof's own device arenas, from ONE place (segment_prover.hip): SegLayout is a pure function of the
// AIRs' shapes, the number of queries and the LogUp flag — no HIP call — and the misc arena is carved by one ordered list of pieces
// that is walked without a base for its size and with the real base for the pointers. The memory policy's `own`, the four
// allocations and the pointers all come from here. Not part of the C ABI.
#pragma once
#include "prover_stages.hpp"

#include <type_traits>

namespace pw {

constexpr size_t kDigestSlack = 16;   // digest records beyond the exact count (offsets and answers)
constexpr size_t kMiscSlack = 8192;   // bytes behind the last piece; the proof-of-work scratch (25 words at `small`) reaches into it

struct SegLayout {
    size_t A = 0;
    uint32_t nq = 0;
    std::vector<size_t> koff;  // where an AIR's openings and gamma powers start among the segment's K_total
    size_t K_total = 0;
    int L = 0;                 // log2 of the tallest LDE
    size_t Nmax = 0, tree_words = 0;
    int n_trees = 0, rounds = 0;
    FriLayout fri;
    // ext arena: FRI layers (2 Nmax) | reduced-opening vectors of the smaller heights (ro_off[k], has_height[k]) | scratch vector (tmp_off)
    std::vector<size_t> ro_off;
    std::vector<char> has_height;
    size_t ext_words = 0, tmp_off = 0;
    size_t cols_total = 0;  // column pointers of the widest matrix per AIR
    size_t row_words = 0;   // query answers: rows of every tree
    size_t n_dig = 0;       // upper bound of the digest records of the query answers (kDigestSlack included)
    size_t dig_bytes = 0, inject_bytes = 0, ext_bytes = 0, misc_bytes = 0;

    SegLayout() : fri(1) {}
    SegLayout(const std::vector<AirShape>& sh, uint32_t nq, bool lg);
    size_t own() const { return dig_bytes + inject_bytes + ext_bytes + misc_bytes; }  // what a call allocates beside its AIRs' buffers
};

// the pieces of the misc arena (8-byte aligned ones first)
struct MiscArena {
    const uint32_t** cols;   // column-pointer table of the tree being hashed
    const uint32_t** sptrs;  // where the AIRs' LogUp sums lie
    GatherRowsJob* jobs;     // query phase: one per AIR and tree
    uint64_t* offs;          // digest | ext | preprocessed-digest offsets
    bb::Ext* opened;
    bb::Ext* gpow;
    uint32_t* idx;           // nq row indices per AIR
    uint32_t* rows;
    uint32_t* dig_out;
    uint32_t* ext_out;
    uint32_t* small;         // 4 A words (the LogUp sums); proof-of-work scratch
    size_t bytes;            // where the walk ended
};

// base == nullptr: sizes only (every pointer null)
inline MiscArena carve_misc(const SegLayout& y, uint8_t* base) {
    size_t off = 0;
    auto take = [&](auto*& piece, size_t n) {
        using T = std::remove_reference_t<decltype(*piece)>;
        piece = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
    };
    const size_t n_ext = (size_t)y.nq * y.rounds;
    MiscArena m{};
    take(m.cols, y.cols_total);
    take(m.sptrs, 4 * y.A);
    take(m.jobs, 4 * y.A);
    take(m.offs, y.n_dig - kDigestSlack + n_ext);
    off += kDigestSlack * 8;
    take(m.opened, y.K_total);
    take(m.gpow, y.K_total);
    take(m.idx, y.A * y.nq);
    take(m.rows, y.row_words);
    take(m.dig_out, (y.n_dig - kDigestSlack) * 8);
    off += kDigestSlack * 32;
    take(m.ext_out, n_ext * 4);
    take(m.small, 4 * y.A);
    off += kMiscSlack;
    m.bytes = off;
    return m;
}

inline SegLayout::SegLayout(const std::vector<AirShape>& sh, uint32_t nq_, bool lg) : A(sh.size()), nq(nq_), koff(sh.size()), fri(1) {
    size_t n_pre_dig = 0;  // the preprocessed trees' siblings (each AIR's own tree)
    for (size_t a = 0; a < A; ++a) {
        koff[a] = K_total;
        K_total += sh[a].K;
        L = std::max(L, sh[a].logN);
        cols_total += std::max<size_t>({sh[a].W, sh[a].Wp, 8});
        row_words += (size_t)nq * sh[a].K1;
        if (sh[a].Wf) n_pre_dig += (size_t)nq * sh[a].logN;
    }
    Nmax = (size_t)1 << L;
    tree_words = merkle_words(Nmax);
    n_trees = lg ? 3 : 2;
    rounds = L - 1;
    fri = FriLayout(L);
    ro_off.assign(L + 1, 0);
    has_height.assign(L + 1, 0);
    for (size_t a = 0; a < A; ++a) has_height[sh[a].logN] = 1;
    ext_words = 2 * Nmax;
    for (int k = L - 1; k >= 2; --k) if (has_height[k]) { ro_off[k] = ext_words; ext_words += (size_t)1 << k; }
    tmp_off = ext_words;
    ext_words += Nmax;
    n_dig = (size_t)nq * ((size_t)n_trees * L + (size_t)rounds * L) + n_pre_dig + kDigestSlack;
    dig_bytes = (n_trees * tree_words + fri.fri_words) * 4;  // three mixed trees | FRI trees
    inject_bytes = (Nmax + 1) * 8 * 4;  // row digests of the heights below Nmax: the slice of height n starts at n * 8 words
    ext_bytes = ext_words * sizeof(bb::Ext);
    misc_bytes = carve_misc(*this, nullptr).bytes;
}

}  // namespace pw
