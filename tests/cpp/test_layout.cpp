// Test-only: the workspace layouts of falcon-r1cs_amd/csrc/frw_layout.h as plain numbers for tests/test_layout_host.py.  Every layout is
// walked from a null base, so a pointer IS its offset; an array a layout does not have is reported as ABSENT.
#include <hip/hip_runtime.h>
#include "frw_layout.h"

using namespace frw;

namespace {
constexpr uint64_t ABSENT = ~0ull;
template <class T> uint64_t off(T *p) { return (uint64_t)(uintptr_t)p; }
size_t bw_of(int group) { return group == 2 ? G2_BK_WORDS : G1_BK_WORDS; }
int put_points(const Groth16Points &p, uint64_t *out)
{
    const uint64_t v[] = {off(p.A), off(p.B1), off(p.L), off(p.H), off(p.SA), off(p.RB1), off(p.B2), off(p.rs), off(p.split)};
    for (int i = 0; i < 9; i++) out[i] = v[i];
    return 9;
}
// the sort's arrays (bare: entry_base first), then a table's own, then end, used, bytes, target, max_items, ones_stride, n
int put_narrow(const NmsmBufs &b, bool bare, uint64_t *out)
{
    const uint64_t v[] = {bare ? off(b.entry_base) : ABSENT, off(b.slice_hist), off(b.counts), off(b.offsets), off(b.item_first), off(b.items), off(b.item_count),
                          off(b.ones_count), off(b.ones_list), off(b.entries), off(b.partial_items), off(b.partial_ones), off(b.folded_ones), off(b.bucket_sums),
                          bare ? off(b.window_sums) : ABSENT, off(b.end), b.used, b.bytes, b.target, b.max_items, b.ones_stride, b.n};
    for (int i = 0; i < 22; i++) out[i] = v[i];
    return 22;
}
int put_dense(const MsmBufs &b, uint64_t *out)
{
    const uint64_t v[] = {off(b.counts), off(b.offsets), off(b.order), off(b.item_first), off(b.item_count), off(b.ones_count), off(b.items), off(b.buckets), off(b.partial),
                          off(b.partial_items), off(b.entries), off(b.ones_list), b.digits ? off(b.digits) : ABSENT, off(b.end),
                          b.window_sums ? off(b.window_sums) : ABSENT, b.bytes, b.max_items, b.ent_stride, b.ones_stride};
    for (int i = 0; i < 19; i++) out[i] = v[i];
    return 19;
}
}  // namespace

extern "C" {
void t_dense(int group, uint64_t rows, uint32_t n, int bare, uint64_t *out) { put_dense(msm_layout(nullptr, rows, n, bare != 0, bw_of(group)), out); }
void t_wide(int group, uint32_t n, uint64_t *out)
{
    const MsmWideBufs w = msm_layout_wide(nullptr, n, bw_of(group));
    out += put_dense(w.rows, out);
    const uint64_t v[] = {off(w.partial_plain), off(w.s1), off(w.s0), off(w.window_sums), off(w.row_start), off(w.bin_start), off(w.row_count), off(w.bin_count),
                          off(w.slice_hist), off(w.coarse), off(w.entries), off(w.digits), off(w.end), w.bytes};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}
void t_narrow(int group, uint64_t cnt, uint32_t n, uint64_t *out) { put_narrow(nmsm_layout(nullptr, cnt, n, bw_of(group)), false, out); }
// sorted: the own arrays only, beside a G1 sort for one table that was laid out at `sort_base`
void t_narrow_bare(int group, uint64_t tables, uint32_t n, int sorted, uint64_t sort_base, uint64_t *out)
{
    const NmsmBufs s = nmsm_layout_bare((void *)(uintptr_t)sort_base, 1, n, G1_BK_WORDS);
    put_narrow(sorted ? nmsm_layout_bare(nullptr, tables, n, bw_of(group), &s) : nmsm_layout_bare(nullptr, tables, n, bw_of(group)), true, out);
}
// dense, dense bare, dense wide, narrow, narrow bare
void t_per_signature(int group, uint32_t n, uint64_t *out)
{
    const size_t bw = bw_of(group);
    out[0] = msm_workspace_per_signature(n, false, false, bw);
    out[1] = msm_workspace_per_signature(n, true, false, bw);
    out[2] = msm_workspace_per_signature(n, true, true, bw);
    out[3] = nmsm_workspace_per_signature(n, false, bw);
    out[4] = nmsm_workspace_per_signature(n, true, bw);
}
uint64_t t_points(uint64_t cnt, uint64_t *out)
{
    Carve c(nullptr);
    put_points(groth16_points_layout(c, cnt), out);
    return c.off;
}
uint64_t t_points_bytes() { return GROTH16_POINTS_BYTES; }
// qap_ws, h, zext, msm_ws[5], the nine points; returns .bytes
uint64_t t_groth16(uint64_t cnt, uint64_t qap, uint64_t domain, uint64_t nv, const uint64_t *msm, uint64_t *out)
{
    const size_t m[5] = {(size_t)msm[0], (size_t)msm[1], (size_t)msm[2], (size_t)msm[3], (size_t)msm[4]};
    const Groth16Bufs g = groth16_layout(nullptr, cnt, qap, domain, nv, m);
    out[0] = off(g.qap_ws); out[1] = off(g.h); out[2] = off(g.zext);
    for (int i = 0; i < 5; i++) out[3 + i] = off(g.msm_ws[i]);
    put_points(g.pts, out + 8);
    return g.bytes;
}
// first_ws, h, zext, where g1, gb and g2 start (their first own array: g2 has no others), the nine points, the three layouts' `used`; returns .bytes
uint64_t t_groth16_bare(uint64_t qap, uint64_t msm_h, uint64_t domain, uint64_t nv, uint32_t nz, uint32_t b_rows, uint64_t *out)
{
    const Groth16BareBufs g = groth16_layout_bare(nullptr, qap, msm_h, domain, nv, nz, b_rows);
    out[0] = off(g.first_ws); out[1] = off(g.h); out[2] = off(g.zext);
    out[3] = off(g.sides.g1.entry_base); out[4] = off(g.sides.gb.entry_base); out[5] = off(g.sides.g2.partial_items);
    put_points(g.pts, out + 6);
    out[15] = g.sides.g1.used; out[16] = g.sides.gb.used; out[17] = g.sides.g2.used;
    out[18] = g.sides.g2.entry_base == g.sides.gb.entry_base && g.sides.g2.entries == g.sides.gb.entries;      // g2 reads gb's sort
    return g.bytes;
}
// decoded, decode_status, msm_ws, prepared, status, pairing_ws, msm_bytes; returns .bytes
uint64_t t_verify(uint64_t k, uint64_t msm_per, int bare, uint64_t proof_bytes, uint64_t pass_bytes, int wire, uint64_t *out)
{
    const VerifyBufs v = verify_layout(nullptr, k, msm_per, bare != 0, proof_bytes, pass_bytes, wire != 0);
    out[0] = wire ? off(v.decoded) : ABSENT; out[1] = wire ? off(v.decode_status) : ABSENT;
    out[2] = off(v.msm_ws); out[3] = off(v.prepared); out[4] = off(v.status); out[5] = off(v.pairing_ws); out[6] = v.msm_bytes;
    return v.bytes;
}
uint64_t t_in_flight(uint64_t batch, uint64_t bytes, uint64_t msm_per, int bare, uint64_t proof_bytes, uint64_t pass_bytes, int wire)
{
    return proofs_in_flight(batch, bytes, [&](size_t k) { return verify_layout(nullptr, k, msm_per, bare != 0, proof_bytes, pass_bytes, wire != 0).bytes; });
}
}
