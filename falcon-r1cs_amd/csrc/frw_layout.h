// frw_layout.h -- where the arrays of every caller-allocated device workspace live: the MSMs', the Groth16 prover's, the verification
// chains'.  One function per layout: it walks the workspace once and returns the pointers; the size a caller is told is the same walk
// from a null base.  Host code only, nothing of the HIP runtime is called: tests/test_layout_host.py compiles this header with g++ and
// checks every offset against tests/golden/workspace_layouts.json.  The sizes and offsets are ABI: callers
// allocate by them, and the alignment of a buffer moves kernel timings.  The constants the layouts depend on are here for that reason;
// what they mean to the kernels is told where the kernels are (frw_msm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace frw {

// walks a workspace: take() hands out the next piece and steps over it, rounded up to `align` bytes (base = nullptr: only sizes)
struct Carve {
    char *base;
    size_t off = 0;
    explicit Carve(void *b) : base((char *)b) {}
    template <class T = void>
    T *take(size_t bytes, size_t align = 256)
    {
        T *p = (T *)(base + off);
        off += (bytes + align - 1) & ~(align - 1);
        return p;
    }
    uint32_t *words(size_t count) { return take<uint32_t>(count * 4, 4); }
    void *at() const { return base + off; }
    void align_to(size_t a) { off = (off + a - 1) & ~(a - 1); }       // (of the offset: every entry point checks its base)
    static size_t up(size_t bytes, size_t a) { return (bytes + a - 1) & ~(a - 1); }
};

constexpr int MSM_C = 16;                       // window bits
constexpr int MSM_W = 16;                       // windows: 16 x 16 = 256 >= 255 bits
constexpr int MSM_BUCKETS = 1 << (MSM_C - 1);   // signed digits: |d| in 1 .. 2^15
constexpr int MSM_FOLD1_THREADS = 4096;         // partial sums per signature at most (first stage: 8, 32 or 64 buckets per thread)
constexpr int G1_BK_WORDS = 60, G2_BK_WORDS = 116;      // words of a bucket (Grp<F>::BK_WORDS): X, Y, ZZ, ZZZ limbs + the infinity flag
constexpr int MSM_SLICES = 32, MSM_SLICES_LONE = 224;
constexpr int WIDE_C = 20, WIDE_W = 13, WIDE_H = 1 << (WIDE_C - MSM_C), WIDE_ROWS = WIDE_W * WIDE_H;
constexpr uint32_t WIDE_MAX_ITEMS = 65536;       // >= 32,768 + (32,768 / 1.5) 33 / 32 (finer = 1)
constexpr int WIDE_SLICES = 128;                 // slices of a window in the bins' sort (whole tiles each)
constexpr int WIDE_BINS = 512, WIDE_BIN_BUCKETS = MSM_BUCKETS * WIDE_H / WIDE_BINS, WIDE_ALL_BINS = WIDE_W * WIDE_BINS, WIDE_TILE = 4096;
constexpr int WIDE_PARTS = 32;
constexpr int MSM_MAX_ITEMS = 131072;          // >= 32,768 + 32,768 / (1.5 / 4): the finest split (a lone signature), a multiple of 64
constexpr int MSM_MAX_ITEMS_LARGE = 32768 + (32768 * 24 * 2 / 3) / 32 * 33 + 64;     // 573,504
static_assert(MSM_MAX_ITEMS_LARGE % 64 == 0 && MSM_MAX_ITEMS >= 32768 + (32768 * 4 * 2 / 3) / 32 * 33 + 64, "whole wavefronts; the finest split fits");
// a bare handle's rows are windows of one sum: sixteen of them fill the chip with items of the buckets' own size (finer = 1)
__host__ __device__ constexpr uint32_t msm_max_items(uint32_t n, bool bare = false)
{
    return !bare && n > (1u << 18) ? (uint32_t)MSM_MAX_ITEMS_LARGE : (uint32_t)MSM_MAX_ITEMS;
}
constexpr int NMSM_C = 8, NMSM_W = 32, NMSM_BUCKETS = 128;
__host__ __device__ constexpr uint32_t nmsm_slices(uint32_t n) { return n > (1u << 18) ? 128u : 16u; }
constexpr int NMSM_TARGET_ITEMS_MIN = 2048, NMSM_TARGET_ITEMS_MAX = 65536;
__host__ __device__ constexpr uint32_t nmsm_target_items(uint32_t n)
{
    const uint32_t t = (n / 128 + 2047) / 2048 * 2048;
    return t < (uint32_t)NMSM_TARGET_ITEMS_MIN ? (uint32_t)NMSM_TARGET_ITEMS_MIN : t > (uint32_t)NMSM_TARGET_ITEMS_MAX ? (uint32_t)NMSM_TARGET_ITEMS_MAX : t;
}
__host__ __device__ constexpr uint32_t nmsm_max_items(uint32_t n) { return nmsm_target_items(n) + 256; }
constexpr int NMSM_ONES_MAX = 4096, NMSM_ONES_MAX_LARGE = 65536;
__host__ __device__ constexpr uint32_t nmsm_ones_max(uint32_t n) { return n > (1u << 18) ? (uint32_t)NMSM_ONES_MAX_LARGE : (uint32_t)NMSM_ONES_MAX; }

// ---- the dense pipeline: per grid row (a signature; a bare handle: a window), every array but the last two a multiple of four words per
// row, so that whatever the number of points everything before them is 16-byte aligned (the items are read two words at a time).
// `bw`: the group's words per bucket.  The sort's per-slice histograms borrow `buckets` (a lone row: `partial_items`) before either is written.
static_assert((size_t)MSM_SLICES * 4 <= (size_t)G1_BK_WORDS * 4, "the slice histograms borrow the buckets' memory");
static_assert((size_t)MSM_SLICES_LONE * MSM_BUCKETS <= (size_t)MSM_MAX_ITEMS * G1_BK_WORDS, "... or, for a lone signature, the work items'");
struct MsmBufs {
    uint32_t *counts, *offsets, *order, *item_first, *item_count, *ones_count, *items, *buckets, *partial, *partial_items, *entries, *ones_list, *end;
    int16_t *digits;            // a bare handle: int16[16][n], the windows' digits of the scalar vector being summed
    uint32_t *window_sums;      // ... and its sixteen window sums, waiting for Horner's rule
    uint32_t max_items;
    size_t ent_stride, ones_stride, bytes;
};
// counts .. partial: what the wide layout shares with the dense one (b.max_items is set)
inline void msm_layout_head(Carve &c, MsmBufs &b, size_t rows, size_t bw)
{
    b.counts = c.words(rows * MSM_BUCKETS); b.offsets = c.words(rows * MSM_BUCKETS);
    b.order = c.words(rows * MSM_BUCKETS); b.item_first = c.words(rows * MSM_BUCKETS);
    b.item_count = c.words(rows * 4); b.ones_count = c.words(rows * 4);         // [rows], four words each
    b.items = c.words(rows * (size_t)b.max_items * 2);                 // [rows][max_items][2]
    b.buckets = c.words(rows * (size_t)MSM_BUCKETS * bw);
    b.partial = c.words(rows * (size_t)MSM_FOLD1_THREADS * bw);
}
inline MsmBufs msm_layout(void *ws, size_t rows, uint32_t n, bool bare, size_t bw)
{
    MsmBufs b{};
    Carve c(ws);
    b.max_items = msm_max_items(n, bare);
    b.ent_stride = bare ? (size_t)n : (size_t)MSM_W * n;
    b.ones_stride = bare ? 0 : (size_t)n;                               // a bare handle's ones are digits like any other
    msm_layout_head(c, b, rows, bw);
    b.partial_items = c.words(rows * (size_t)b.max_items * bw);
    b.entries = c.words(rows * b.ent_stride);
    b.ones_list = c.words(rows * b.ones_stride);
    if (bare) b.digits = (int16_t *)c.words(((size_t)MSM_W * n * 2 + 3) / 4);
    b.end = (uint32_t *)c.at();
    if (bare) { c.align_to(16); b.window_sums = c.words((size_t)MSM_W * bw); }
    b.bytes = Carve::up(c.off, 16);
    return b;
}
// thirteen 20-bit windows (WIDE_*): 208 rows.  The parts' histograms borrow `rows.buckets`, the digits `entries` (dead once the bins are
// sorted; the entries are written after that).
struct MsmWideBufs {
    MsmBufs rows;                       // the 208 rows' arrays (entries apart: below)
    uint32_t *partial_plain, *slice_hist, *bin_count, *row_count, *s1, *s0, *window_sums, *entries, *end;
    unsigned long long *row_start, *bin_start;
    uint2 *coarse;
    int32_t *digits;
    size_t bytes;
};
inline MsmWideBufs msm_layout_wide(void *ws, uint32_t n, size_t bw)
{
    constexpr size_t R = WIDE_ROWS;
    MsmWideBufs w{};
    MsmBufs &b = w.rows;
    Carve c(ws);
    b.max_items = WIDE_MAX_ITEMS;
    msm_layout_head(c, b, R, bw);
    w.partial_plain = c.words(R * (size_t)MSM_FOLD1_THREADS * bw);
    b.partial_items = c.words(R * (size_t)b.max_items * bw);
    w.s1 = c.words(R * bw); w.s0 = c.words(R * bw);
    w.window_sums = c.words((size_t)WIDE_W * bw);
    w.row_start = c.take<unsigned long long>(R * 8, 8);                 // (every term so far a multiple of four words)
    w.bin_start = c.take<unsigned long long>((size_t)WIDE_ALL_BINS * 8, 8);
    w.row_count = c.words(R); w.bin_count = c.words(WIDE_ALL_BINS);
    w.slice_hist = c.words((size_t)WIDE_W * WIDE_SLICES * WIDE_BINS);
    w.coarse = (uint2 *)c.words((size_t)WIDE_W * n * 2);
    w.entries = c.words((size_t)WIDE_W * n);
    w.digits = (int32_t *)w.entries;
    w.end = (uint32_t *)c.at();
    b.entries = w.entries; b.ones_list = w.end; b.end = w.end;
    w.bytes = Carve::up(c.off, 16);
    return w;
}
// what frw_msm_info reports for a dense handle (a bare one: sixteen rows, the windows, and their sixteen sums)
inline size_t msm_workspace_per_signature(uint32_t n, bool bare, bool wide, size_t bw)
{
    return wide ? msm_layout_wide(nullptr, n, bw).bytes : msm_layout(nullptr, bare ? MSM_W : 1, n, bare, bw).bytes;
}

// ---- the narrow pipeline: the sort's arrays (which know nothing of the points) and a table's own
struct NmsmBufs {
    uint32_t *slice_hist, *counts, *offsets, *item_first, *items, *item_count, *ones_count, *ones_list, *entries;      // the sort's
    uint32_t *partial_items, *partial_ones, *folded_ones, *bucket_sums;                                              // a table's own
    uint32_t target, max_items, ones_stride;
    uint32_t n = 0;             // (bare) how many scalars the sort is over: a table's rows, or the rows its index names
    // a bare handle's sort (rows = the thirty-two windows of one scalar vector): where every window's entries start, and its tables'
    // window sums [table][32]
    unsigned long long *entry_base = nullptr;
    uint32_t *window_sums = nullptr;
    uint32_t *end = nullptr;
    size_t used = 0, bytes = 0;      // from the base to `end`; what frw_msm_info reports for one signature
};
// a window table's: slice histograms, counts, offsets, first item of every bucket (all x 128), the item list + counter, the ones' list +
// counter, the entries (32 n x 4 B), the items' and the ones' partial sums
inline NmsmBufs nmsm_layout(void *ws, size_t cnt, uint32_t n, size_t bw)
{
    NmsmBufs b;
    Carve c(ws);
    b.target = nmsm_target_items(n); b.max_items = nmsm_max_items(n); b.ones_stride = nmsm_ones_max(n) / 64;
    b.slice_hist = c.words(cnt * (size_t)nmsm_slices(n) * NMSM_BUCKETS);
    b.counts = c.words(cnt * NMSM_BUCKETS);
    b.offsets = c.words(cnt * NMSM_BUCKETS);
    b.item_first = c.words(cnt * NMSM_BUCKETS);
    b.items = c.words(cnt * (size_t)b.max_items);
    b.item_count = c.words(cnt * 4);                                    // [cnt], four words per signature
    b.ones_count = c.words(cnt * 4);                                    // likewise
    b.ones_list = c.words(cnt * (size_t)n);
    b.entries = c.words(cnt * (size_t)NMSM_W * n);
    c.align_to(16);                                                     // every term above is a multiple of 4 words per signature but n: at most three words
    b.partial_items = c.words(cnt * (size_t)b.max_items * bw);
    b.partial_ones = c.words(cnt * (size_t)b.ones_stride * bw);
    b.folded_ones = c.words(b.ones_stride > 64 ? cnt * (size_t)64 * bw : 0);     // second stage, only when ones_stride > 64
    b.bucket_sums = c.words(cnt * (size_t)NMSM_BUCKETS * bw);
    b.end = (uint32_t *)c.at();
    b.used = c.off;
    b.bytes = Carve::up(c.off + 16, 16);        // four words more than the arrays: the pad above was budgeted apart from them, and the sum is what callers were told
    return b;
}
// ... of a bare handle: ONE sort (thirty-two window rows) and the own arrays of `tables` tables.  The entries are budgeted for the worst
// case, every digit of every scalar non-zero (32 n words); a witness fills a seventieth of that.
// `sorted`: another layout whose sort this one reads (the G2 sum of a proof reads the G1 sums' sort): only the own arrays are laid out then.
inline NmsmBufs nmsm_layout_bare(void *ws, size_t tables, uint32_t n, size_t bw, const NmsmBufs *sorted = nullptr)
{
    constexpr size_t WIN = NMSM_W;
    NmsmBufs b;
    Carve c(ws);
    if (sorted) {
        b = *sorted;
    } else {
        b.target = nmsm_target_items(n); b.max_items = nmsm_max_items(n); b.ones_stride = nmsm_ones_max(n) / 64; b.n = n;
        b.entry_base = c.take<unsigned long long>(WIN * 8, 8);             // [32]
        b.slice_hist = c.words(WIN * (size_t)nmsm_slices(n) * NMSM_BUCKETS);
        b.counts = c.words(WIN * NMSM_BUCKETS);
        b.offsets = c.words(WIN * NMSM_BUCKETS);
        b.item_first = c.words(WIN * NMSM_BUCKETS);
        b.items = c.words(WIN * (size_t)b.max_items);
        b.item_count = c.words(WIN * 4);
        b.ones_count = c.words(4);                                         // [0] is the one in use (every term so far a multiple of four words)
    }
    b.partial_items = c.words(tables * WIN * (size_t)b.max_items * bw);
    b.partial_ones = c.words(tables * (size_t)b.ones_stride * bw);
    b.folded_ones = c.words(tables * (size_t)64 * bw);
    b.bucket_sums = c.words(tables * WIN * (size_t)NMSM_BUCKETS * bw);
    b.window_sums = c.words(tables * WIN * bw);
    if (!sorted) {
        b.ones_list = c.words(n);
        b.entries = c.words(WIN * (size_t)n);
    }
    b.end = (uint32_t *)c.at();
    b.used = c.off;
    b.bytes = Carve::up(c.off + 16, 16);        // (the window tables' four words more, here too: reported so since bare handles exist)
    return b;
}
inline size_t nmsm_workspace_per_signature(uint32_t n, bool bare, size_t bw) { return bare ? nmsm_layout_bare(nullptr, 1, n, bw).bytes : nmsm_layout(nullptr, 1, n, bw).bytes; }

// ---- the Groth16 prover.  The points of `cnt` proofs: [A | B1' | L] [H] [s A | r B1'] (G1, XYZZ: 240 bytes each), B (G2, affine), r and
// s, and their split halves
struct Groth16Points { uint32_t *A, *B1, *L, *H, *SA, *RB1; uint64_t *B2, *rs, *split; };
constexpr size_t GROTH16_POINTS_BYTES = 6 * (size_t)G1_BK_WORDS * 4 + 192 + 64 + 64;      // (of one proof: tests/test_layout_host.py holds the layout to it)
inline Groth16Points groth16_points_layout(Carve &c, size_t cnt)
{
    Groth16Points p;
    p.A = c.words(cnt * G1_BK_WORDS); p.B1 = c.words(cnt * G1_BK_WORDS); p.L = c.words(cnt * G1_BK_WORDS);
    p.H = c.words(cnt * G1_BK_WORDS); p.SA = c.words(cnt * G1_BK_WORDS); p.RB1 = c.words(cnt * G1_BK_WORDS);
    p.B2 = c.take<uint64_t>(cnt * 192, 8); p.rs = c.take<uint64_t>(cnt * 64, 8); p.split = c.take<uint64_t>(cnt * 64, 8);
    return p;
}
// One chunk of `cnt` proofs with a key of window tables: the witness map's workspace, h, z ++ [1, r, s], the five sums' workspaces
// (h_query, a_query, b_g1_query, l_query, b_g2_query: each its own, they overlap in time), the points.
// qap, msm[]: bytes per signature as frw_qap_info / frw_msm_info report them.
// .qap, .msm[]: per proof (the sums' rounded up to 256); .bytes with cnt = 1: the workspace of one proof in flight
struct Groth16Bufs { void *qap_ws; uint64_t *h, *zext; char *msm_ws[5]; Groth16Points pts; size_t qap, msm[5], bytes; };
inline Groth16Bufs groth16_layout(void *ws, size_t cnt, size_t qap, size_t domain, size_t nv, const size_t *msm)
{
    Groth16Bufs g{};
    Carve c(ws);
    g.qap = qap;
    g.qap_ws = c.take(cnt * qap, 1);
    g.h = c.take<uint64_t>(cnt * domain * 32, 1);
    g.zext = c.take<uint64_t>(cnt * (nv + 3) * 32, 1);
    for (int i = 0; i < 5; i++) { g.msm[i] = Carve::up(msm[i], 256); g.msm_ws[i] = c.take<char>(cnt * g.msm[i], 1); }
    g.pts = groth16_points_layout(c, cnt);
    g.bytes = Carve::up(c.off, 256);
    return g;
}
// The witness-side sums of a key of bare handles: g1, the sort of the slice's `nz` scalars and the own arrays of a_query and l_query; gb,
// the sort of the scalars of the `b_rows` rows b_g1_query / b_g2_query hold a point in and b_g1_query's own arrays; g2, b_g2_query's own
// arrays (it reads gb's sort).  Each is rounded up to 256 bytes.
struct Groth16Sides { NmsmBufs g1, gb, g2; };
inline Groth16Sides groth16_sides_layout(Carve &c, uint32_t nz, uint32_t b_rows)
{
    Groth16Sides s;
    s.g1 = nmsm_layout_bare(c.at(), 2, nz, G1_BK_WORDS);              c.take(s.g1.used);
    s.gb = nmsm_layout_bare(c.at(), 1, b_rows, G1_BK_WORDS);          c.take(s.gb.used);
    s.g2 = nmsm_layout_bare(c.at(), 1, b_rows, G2_BK_WORDS, &s.gb);   c.take(s.g2.used);
    return s;
}
// One proof with a key of bare handles.  The witness map's workspace and the sum over h_query's are ONE region: the sum starts, on the
// same stream, when the map is through and has left h -- 30 GB of the 2^27 domain's workspace.
// first_ws: the witness map's, then the sum over h_query's; .qap, .msm_h: their sizes, rounded up to 256
struct Groth16BareBufs { void *first_ws; uint64_t *h, *zext; Groth16Sides sides; Groth16Points pts; size_t qap, msm_h, bytes; };
inline Groth16BareBufs groth16_layout_bare(void *ws, size_t qap, size_t msm_h, size_t domain, size_t nv, uint32_t nz, uint32_t b_rows)
{
    Groth16BareBufs g{};
    Carve c(ws);
    g.qap = Carve::up(qap, 256); g.msm_h = Carve::up(msm_h, 256);
    g.first_ws = c.take(g.qap > g.msm_h ? g.qap : g.msm_h, 1);
    g.h = c.take<uint64_t>(domain * 32, 1);
    g.zext = c.take<uint64_t>((nv + 3) * 32, 1);
    g.sides = groth16_sides_layout(c, nz, b_rows);
    g.pts = groth16_points_layout(c, 1);
    g.bytes = Carve::up(c.off, 256);
    return g;
}

// ---- the verification chains, `k` proofs in flight: (from the wire format: the decoded proofs, 384 bytes each, and the decoder's
// statuses,) the sum's workspace -- one vector's for a bare handle --, the prepared points and the statuses, (on the device: the pairing's
// per proof and per pass).  msm_per: what frw_msm_info reports for the key's handle, a multiple of 16.
struct VerifyBufs { uint64_t *decoded, *prepared; int32_t *decode_status, *status; void *msm_ws, *pairing_ws; size_t msm_bytes, bytes; };
inline VerifyBufs verify_layout(void *ws, size_t k, size_t msm_per, bool bare, size_t proof_bytes = 0, size_t pass_bytes = 0, bool wire = false)
{
    VerifyBufs v{};
    Carve c(ws);
    if (wire) { v.decoded = c.take<uint64_t>(384 * k, 8); v.decode_status = c.take<int32_t>(4 * k, 16); }
    v.msm_bytes = msm_per * (bare ? 1 : k);
    v.msm_ws = c.take(v.msm_bytes, 1);
    v.prepared = c.take<uint64_t>(96 * k, 8);
    v.status = c.take<int32_t>(4 * k, 16);
    v.pairing_ws = c.take(k * proof_bytes + pass_bytes, 1);
    v.bytes = c.off;
    return v;
}
// ---- re-randomising proofs (frw_rerand.hip), `k` proofs in flight: the sixteen scalar words of a proof (the split halves of r1^-1 and
// r2, then r1 and r1 r2), A' and C' as the ladders leave them (G1, XYZZ: two buckets a proof), B' likewise (G2), and for the wire form
// the decoded limbs, which the chain re-randomises in place, with the decoder's and the encoder's statuses.  The proofs' own statuses
// live in the caller's array.  Every piece is rounded up to 16 bytes.
struct RerandBufs { uint64_t *scalars; uint32_t *g1_points, *g2_points; uint64_t *decoded; int32_t *decode_status, *encode_status; size_t bytes; };
constexpr size_t RERAND_SCALAR_BYTES = 128;
inline RerandBufs rerand_layout(void *ws, size_t k, bool wire)
{
    RerandBufs b{};
    Carve c(ws);
    b.scalars = c.take<uint64_t>(k * RERAND_SCALAR_BYTES, 16);
    b.g1_points = c.take<uint32_t>(k * 2 * (size_t)G1_BK_WORDS * 4, 16);
    b.g2_points = c.take<uint32_t>(k * (size_t)G2_BK_WORDS * 4, 16);
    if (wire) {
        b.decoded = c.take<uint64_t>(k * 384, 16);
        b.decode_status = c.take<int32_t>(k * 4, 16);
        b.encode_status = c.take<int32_t>(k * 4, 16);
    }
    b.bytes = c.off;
    return b;
}
// ---- the verifier's statement from bytes (frw_statement_from_bytes_dev): the decoded public keys and the hashed messages as uint16_t
// [batch][N] each, 16-byte aligned, and the key decoder's statuses, which the statement kernel reads before it looks at a coefficient
struct StatementBufs { uint16_t *pk, *hm; int32_t *decode_status; size_t bytes; };
inline StatementBufs statement_layout(void *ws, int logn, size_t batch)
{
    StatementBufs b{};
    Carve c(ws);
    b.pk = c.take<uint16_t>((batch << logn) * 2, 16);
    b.hm = c.take<uint16_t>((batch << logn) * 2, 16);
    b.decode_status = c.take<int32_t>(batch * 4, 16);
    b.bytes = c.off;
    return b;
}
// ---- Falcon verification from bytes (frw_falcon_verify_from_bytes_dev): the decoded signatures, the decoded public keys and the hashed
// messages as uint16_t[batch][N] each, the signatures' nonces as batch x 40 bytes, then the signature decoder's and the key decoder's
// int32_t[batch] statuses, which the kernel reads before it looks at a coefficient; every piece rounded up to 16 bytes
struct FalconVerifyBufs { uint16_t *sig, *pk, *hm; uint8_t *nonce; int32_t *sig_status, *pk_status; size_t bytes; };
inline FalconVerifyBufs falcon_verify_layout(void *ws, int logn, size_t batch)
{
    FalconVerifyBufs b{};
    Carve c(ws);
    b.sig = c.take<uint16_t>((batch << logn) * 2, 16);
    b.pk = c.take<uint16_t>((batch << logn) * 2, 16);
    b.hm = c.take<uint16_t>((batch << logn) * 2, 16);
    b.nonce = c.take<uint8_t>(batch * 40, 16);
    b.sig_status = c.take<int32_t>(batch * 4, 16);
    b.pk_status = c.take<int32_t>(batch * 4, 16);
    b.bytes = c.off;
    return b;
}
// ---- the prover from bytes (frw_pok_prove_from_bytes_dev).  A fixed part proportional to `batch`: the screen's own workspace (the
// layout above: decoded arrays, nonces, both decoders' statuses), the accepted slots' indices in slot order, one word per block of
// POK_SCAN_BLOCK slots for the scan, the count (a piece of 16 bytes: the one value the host reads), and the accepted slots' blinding
// factors, dense.  Then, from a 256-byte boundary, `k` times a per-signature part -- the witness (num_witness elements), the instance
// vector, the gathered sig, pk, hm rows, the proof's limbs, its wire bytes (384: the longer mode's, the size does not depend on the
// mode), the witness kernel's and the encoder's status words and the prover's count of violated rows -- and, 256-byte aligned again, the
// Groth16 prover's workspace for k proofs in flight (groth16_bytes = frw_groth16_workspace_bytes(pk, r, k)).  Every piece is rounded up to
// 16 bytes at least.
constexpr size_t POK_SCAN_BLOCK = 256;           // slots per workgroup of the scan kernels (== BLOCK of frw_device.h)
constexpr size_t POK_WIRE_STAGE = 384;           // staged wire bytes per proof: FRW_WIRE_UNCOMPRESSED's
struct PokProveBufs {
    FalconVerifyBufs screen;
    uint32_t *index, *block_sums, *count;
    uint64_t *rs;
    uint64_t *witness, *instance;
    uint16_t *sig, *pk, *hm;
    uint64_t *proofs;
    uint8_t *wire;
    int32_t *witness_status, *wire_status;
    uint32_t *unsatisfied;
    void *groth16_ws;
    size_t fixed_bytes, per_signature_bytes, groth16_bytes, bytes;
};
inline PokProveBufs pok_prove_layout(void *ws, int logn, size_t batch, size_t k, size_t num_witness, size_t groth16_bytes)
{
    PokProveBufs b{};
    Carve c(ws);
    const size_t n = (size_t)1 << logn;
    b.screen = falcon_verify_layout(c.at(), logn, batch);
    c.take(b.screen.bytes, 16);
    b.index = c.take<uint32_t>(batch * 4, 16);
    b.block_sums = c.take<uint32_t>((batch + POK_SCAN_BLOCK - 1) / POK_SCAN_BLOCK * 4, 16);
    b.count = c.take<uint32_t>(16, 16);
    b.rs = c.take<uint64_t>(batch * 64, 16);
    b.fixed_bytes = c.off;
    c.align_to(256);
    const size_t per0 = c.off;
    b.witness = c.take<uint64_t>(k * num_witness * 32, 256);
    b.instance = c.take<uint64_t>(k * (2 * n + 1) * 32, 16);
    b.sig = c.take<uint16_t>(k * n * 2, 16);
    b.pk = c.take<uint16_t>(k * n * 2, 16);
    b.hm = c.take<uint16_t>(k * n * 2, 16);
    b.proofs = c.take<uint64_t>(k * 384, 16);
    b.wire = c.take<uint8_t>(k * POK_WIRE_STAGE, 16);
    b.witness_status = c.take<int32_t>(k * 4, 16);
    b.wire_status = c.take<int32_t>(k * 4, 16);
    b.unsatisfied = c.take<uint32_t>(k * 4, 16);
    b.per_signature_bytes = c.off - per0;          // (of all k)
    c.align_to(256);
    b.groth16_ws = c.take(groth16_bytes, 256);
    b.groth16_bytes = groth16_bytes;
    b.bytes = c.off;
    return b;
}
// ---- an aggregate's inputs from bytes (frw_aggregate_*_from_bytes_dev).  The encoded keys, and the encoded signatures, of the statements
// lie end to end in STATEMENT order, Falcon-512 and Falcon-1024 mixed (set g = logn - 9): 897 | 1,793 bytes a key, 666 | 1,280 a signature,
// so nothing is aligned.  Item k of set g is the k-th statement of that set, statement s of the aggregate (R1csAggSet::stmt): k statements
// of its own set and s - k of the other one lie before it.  The nonces are 40 bytes a statement, in statement order.  This one function is
// where the kernels (frw_prepare.hip), the size functions and the host-side staging (frw_stage.h) get it from.
__host__ __device__ constexpr size_t aggregate_pk_len(int g) { return g ? 1793 : 897; }        // FRW_PK_LEN(9 + g)
__host__ __device__ constexpr size_t aggregate_sig_len(int g) { return g ? 1280 : 666; }       // FRW_SIG_LEN(9 + g)
struct AggRoute { size_t pk_off, sig_off, nonce_off; };
__host__ __device__ inline AggRoute aggregate_route(int g, size_t k, size_t s)
{
    const size_t other = s - k;
    AggRoute r;
    r.pk_off = k * aggregate_pk_len(g) + other * aggregate_pk_len(g ^ 1);
    r.sig_off = k * aggregate_sig_len(g) + other * aggregate_sig_len(g ^ 1);
    r.nonce_off = s * 40;
    return r;
}
// all the keys' | signatures' bytes of an aggregate of count9 Falcon-512 and count10 Falcon-1024 statements: where statement `count` would start
__host__ __device__ inline size_t aggregate_pk_bytes(size_t count9, size_t count10) { return aggregate_route(0, count9, count9 + count10).pk_off; }
__host__ __device__ inline size_t aggregate_sig_bytes(size_t count9, size_t count10) { return aggregate_route(0, count9, count9 + count10).sig_off; }

// ---- the screen of an aggregate from bytes (frw_aggregate_falcon_verify_from_bytes_dev; frw_aggregate_statement_from_bytes_dev uses the
// pk, hm and pk_status pieces of the same layout).  Per parameter set g, dense in the set's own order: the decoded signatures, keys and
// hashed messages as uint16_t[count_g][N_g], both decoders' statuses, the verification kernel's status words and norms.  Then what is in
// statement order: the nonces, count x 40 bytes, and one piece of 16 bytes for the number of refused statements (the one value the
// prover's host side reads).  Every piece is rounded up to 16 bytes.
struct AggregateScreenBufs {
    uint16_t *sig[2], *pk[2], *hm[2];
    int32_t *sig_status[2], *pk_status[2], *status[2];
    uint64_t *norm[2];
    uint8_t *nonce;
    uint32_t *refused;
    size_t bytes;
};
inline AggregateScreenBufs aggregate_screen_layout(void *ws, size_t count9, size_t count10)
{
    AggregateScreenBufs b{};
    Carve c(ws);
    const size_t count[2] = {count9, count10};
    for (int g = 0; g < 2; g++) {
        const size_t row = count[g] * ((size_t)512 << g) * 2;
        b.sig[g] = c.take<uint16_t>(row, 16);
        b.pk[g] = c.take<uint16_t>(row, 16);
        b.hm[g] = c.take<uint16_t>(row, 16);
        b.sig_status[g] = c.take<int32_t>(count[g] * 4, 16);
        b.pk_status[g] = c.take<int32_t>(count[g] * 4, 16);
        b.status[g] = c.take<int32_t>(count[g] * 4, 16);
        b.norm[g] = c.take<uint64_t>(count[g] * 8, 16);
    }
    b.nonce = c.take<uint8_t>((count9 + count10) * 40, 16);
    b.refused = c.take<uint32_t>(16, 16);
    b.bytes = c.off;
    return b;
}
// ---- the aggregate prover from bytes (frw_aggregate_prove_from_bytes_dev): the screen's layout above; then from a 256-byte boundary,
// per parameter set, the witness kernel's batch (count_g x W_g elements; W = 153 N + 50 | 52), its instance batch (count_g x (2 N + 1))
// and its status words; the aggregate's own witness and instance vectors (sum of W_g count_g; 1 + sum of 2 N_g count_g elements), the
// proof's 48 limbs, 384 wire bytes (the longer mode's), the encoder's status word, the prover's count of violated rows, the status words
// of the statement kernels (statement order; the caller's array holds the screen's); and, 256-byte
// aligned, the Groth16 prover's workspace for the one proof (groth16_bytes = frw_groth16_workspace_bytes(pk, aggregate, 1)).
struct AggregateProveBufs {
    AggregateScreenBufs screen;
    uint64_t *set_witness[2], *set_instance[2];
    int32_t *witness_status[2];
    uint64_t *witness, *instance, *proof;
    uint8_t *wire;
    int32_t *wire_status, *statement_status;
    uint32_t *unsatisfied;
    void *groth16_ws;
    size_t num_witness, num_instance;      // of the aggregate
    size_t groth16_bytes, bytes;
};
inline AggregateProveBufs aggregate_prove_layout(void *ws, size_t count9, size_t count10, size_t groth16_bytes)
{
    AggregateProveBufs b{};
    Carve c(ws);
    const size_t count[2] = {count9, count10};
    b.screen = aggregate_screen_layout(c.at(), count9, count10);
    c.take(b.screen.bytes, 256);
    b.num_instance = 1;
    for (int g = 0; g < 2; g++) {
        const size_t n = (size_t)512 << g, W = 153 * n + (g ? 52 : 50), I = 2 * n + 1;
        c.align_to(256);
        b.set_witness[g] = c.take<uint64_t>(count[g] * W * 32, 256);
        b.set_instance[g] = c.take<uint64_t>(count[g] * I * 32, 16);
        b.witness_status[g] = c.take<int32_t>(count[g] * 4, 16);
        b.num_witness += count[g] * W;
        b.num_instance += count[g] * (I - 1);
    }
    c.align_to(256);
    b.witness = c.take<uint64_t>(b.num_witness * 32, 256);
    b.instance = c.take<uint64_t>(b.num_instance * 32, 16);
    b.proof = c.take<uint64_t>(384, 16);
    b.wire = c.take<uint8_t>(POK_WIRE_STAGE, 16);
    b.wire_status = c.take<int32_t>(4, 16);
    b.unsatisfied = c.take<uint32_t>(4, 16);
    b.statement_status = c.take<int32_t>((count9 + count10) * 4, 16);
    c.align_to(256);
    b.groth16_ws = c.take(groth16_bytes, 256);
    b.groth16_bytes = groth16_bytes;
    b.bytes = c.off;
    return b;
}
// ---- the sum over a run-time curve (frw_msm_field.hip): a chunk of statements, W windows of 2^(C - 1) buckets each ------------------
// keys = W 2^(C - 1) (window, bucket) pairs a statement; a fold level brings MSMF_FOLD (weighted, plain) pairs down to one.
constexpr int MSMF_FOLD_LOG = 3, MSMF_FOLD = 1 << MSMF_FOLD_LOG;
constexpr int MSMF_XYZZ_WORDS = 32;
struct MsmfBufs {
    uint32_t *counts;       // [statements][keys]        entries of a key          (zeroed at the head of a chunk)
    uint32_t *offsets;      // [statements][keys]        where they start in the statement's entries
    uint32_t *cursor;       // [statements][keys]        the scatter's next free place
    uint32_t *entries;      // [statements][W n]         point index | sign << 31
    int16_t *digits;        // [statements][W][n]
    uint32_t *buckets;      // [statements][keys][32]    XYZZ
    uint32_t *fold[2];      // [statements][keys / 8][2][32], [statements][keys / 64][2][32]: the levels alternate
    size_t bytes;
};
inline MsmfBufs msmf_layout(void *ws, size_t statements, size_t n, int window_bits, int windows)
{
    MsmfBufs b{};
    Carve c(ws);
    const size_t keys = (size_t)windows << (window_bits - 1);
    b.counts = c.take<uint32_t>(statements * keys * 4);
    b.offsets = c.take<uint32_t>(statements * keys * 4);
    b.cursor = c.take<uint32_t>(statements * keys * 4);
    b.entries = c.take<uint32_t>(statements * windows * n * 4);
    b.digits = c.take<int16_t>(statements * windows * n * 2);
    b.buckets = c.take<uint32_t>(statements * keys * MSMF_XYZZ_WORDS * 4);
    b.fold[0] = c.take<uint32_t>(statements * (keys >> MSMF_FOLD_LOG) * 2 * MSMF_XYZZ_WORDS * 4);
    b.fold[1] = c.take<uint32_t>(statements * (keys >> 2 * MSMF_FOLD_LOG) * 2 * MSMF_XYZZ_WORDS * 4);
    b.bytes = c.off;
    return b;
}
// ---- the same sum over a curve on a run-time Fq2 (frw_msm_field2.hip): the schedule and the scalar side are msmf_layout's, an XYZZ
// item is four Fe2 = 64 words -------------------------------------------------------------------------------------------------------
constexpr int MSMF2_XYZZ_WORDS = 64;
struct Msmf2Bufs {
    uint32_t *counts;       // [statements][keys]
    uint32_t *offsets;      // [statements][keys]
    uint32_t *cursor;       // [statements][keys]
    uint32_t *entries;      // [statements][W n]         point index | sign << 31
    int16_t *digits;        // [statements][W][n]
    uint32_t *buckets;      // [statements][keys][64]    XYZZ over Fe2
    uint32_t *fold[2];      // [statements][keys / 8][2][64], [statements][keys / 64][2][64]: the levels alternate
    size_t bytes;
};
inline Msmf2Bufs msmf2_layout(void *ws, size_t statements, size_t n, int window_bits, int windows)
{
    Msmf2Bufs b{};
    Carve c(ws);
    const size_t keys = (size_t)windows << (window_bits - 1);
    b.counts = c.take<uint32_t>(statements * keys * 4);
    b.offsets = c.take<uint32_t>(statements * keys * 4);
    b.cursor = c.take<uint32_t>(statements * keys * 4);
    b.entries = c.take<uint32_t>(statements * windows * n * 4);
    b.digits = c.take<int16_t>(statements * windows * n * 2);
    b.buckets = c.take<uint32_t>(statements * keys * MSMF2_XYZZ_WORDS * 4);
    b.fold[0] = c.take<uint32_t>(statements * (keys >> MSMF_FOLD_LOG) * 2 * MSMF2_XYZZ_WORDS * 4);
    b.fold[1] = c.take<uint32_t>(statements * (keys >> 2 * MSMF_FOLD_LOG) * 2 * MSMF2_XYZZ_WORDS * 4);
    b.bytes = c.off;
    return b;
}

// the most proofs in flight, up to `batch`, whose workspace size(k) fits `bytes` (0: not even one)
template <class SizeFn> size_t proofs_in_flight(size_t batch, size_t bytes, SizeFn size)
{
    if (batch == 0 || size(1) > bytes) return 0;
    size_t lo = 1, hi = batch;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (size(mid) <= bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace frw
