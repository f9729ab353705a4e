// Test-only: the host side of the aggregate from bytes (frw_layout.h aggregate_route, aggregate_screen_layout, aggregate_prove_layout;
// frw_stage.h StagedAggregate).
//   as a shared library (tests/test_aggregate_bytes_abi.py): t_agg_* walk the layouts from a null base, so a pointer IS its offset, and
//   hand the routing function's offsets to Python, which holds them to prefix sums;
//   as a program (the same test builds it with -fsanitize=address,undefined and runs it): main carves real memory of exactly the size
//   each layout reports, fills every piece to its last byte with a value of its own and reads all of them back -- a piece that overlaps
//   a neighbour reads the neighbour's value, one that reaches past the end trips the sanitizer -- and stages mixed-length inputs from
//   sources that are exactly as long as a caller's into a heap buffer of exactly the reported size.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frw_stage.h"

namespace {
constexpr int SCREEN_PIECES = 16, PROVE_PIECES = SCREEN_PIECES + 13;
struct Pieces {
    const void *p[PROVE_PIECES + 1];             // (+ the Groth16 workspace, which main adds)
    size_t len[PROVE_PIECES + 1];
    int n = 0;
    void add(const void *ptr, size_t bytes) { p[n] = ptr; len[n] = bytes; n++; }
};
void screen_pieces(const frw::AggregateScreenBufs &b, size_t c9, size_t c10, Pieces &out)
{
    const size_t count[2] = {c9, c10};
    for (int g = 0; g < 2; g++) {
        const size_t row = count[g] * ((size_t)512 << g) * 2;
        out.add(b.sig[g], row); out.add(b.pk[g], row); out.add(b.hm[g], row);
        out.add(b.sig_status[g], count[g] * 4); out.add(b.pk_status[g], count[g] * 4); out.add(b.status[g], count[g] * 4);
        out.add(b.norm[g], count[g] * 8);
    }
    out.add(b.nonce, (c9 + c10) * 40);
    out.add(b.refused, 4);
}
void prove_pieces(const frw::AggregateProveBufs &b, size_t c9, size_t c10, Pieces &out)
{
    const size_t count[2] = {c9, c10};
    screen_pieces(b.screen, c9, c10, out);
    for (int g = 0; g < 2; g++) {
        const size_t n = (size_t)512 << g, W = 153 * n + (g ? 52 : 50);
        out.add(b.set_witness[g], count[g] * W * 32); out.add(b.set_instance[g], count[g] * (2 * n + 1) * 32);
        out.add(b.witness_status[g], count[g] * 4);
    }
    out.add(b.witness, b.num_witness * 32); out.add(b.instance, b.num_instance * 32);
    out.add(b.proof, 384); out.add(b.wire, 384); out.add(b.wire_status, 4); out.add(b.unsatisfied, 4);
    out.add(b.statement_status, (c9 + c10) * 4);
}
void emit(const Pieces &pc, uint64_t *out)
{
    for (int i = 0; i < pc.n; i++) { out[2 * i] = (uint64_t)(uintptr_t)pc.p[i]; out[2 * i + 1] = pc.len[i]; }
}
}  // namespace

extern "C" {
void t_agg_route(int g, uint64_t k, uint64_t s, uint64_t out[3])
{
    const frw::AggRoute r = frw::aggregate_route(g, k, s);
    out[0] = r.pk_off; out[1] = r.sig_off; out[2] = r.nonce_off;
}
uint64_t t_agg_pk_bytes(uint64_t c9, uint64_t c10) { return frw::aggregate_pk_bytes(c9, c10); }
uint64_t t_agg_sig_bytes(uint64_t c9, uint64_t c10) { return frw::aggregate_sig_bytes(c9, c10); }
int t_agg_screen_pieces(void) { return SCREEN_PIECES; }
int t_agg_prove_pieces(void) { return PROVE_PIECES; }
// out[2 i], out[2 i + 1]: offset and length of piece i; returns .bytes
uint64_t t_agg_screen(uint64_t c9, uint64_t c10, uint64_t *out)
{
    const frw::AggregateScreenBufs b = frw::aggregate_screen_layout(nullptr, c9, c10);
    Pieces pc;
    screen_pieces(b, c9, c10, pc);
    emit(pc, out);
    return b.bytes;
}
// ... then the Groth16 workspace's offset and length, then num_witness and num_instance
uint64_t t_agg_prove(uint64_t c9, uint64_t c10, uint64_t groth16_bytes, uint64_t *out)
{
    const frw::AggregateProveBufs b = frw::aggregate_prove_layout(nullptr, c9, c10, groth16_bytes);
    Pieces pc;
    prove_pieces(b, c9, c10, pc);
    emit(pc, out);
    out[2 * pc.n] = (uint64_t)(uintptr_t)b.groth16_ws; out[2 * pc.n + 1] = b.groth16_bytes;
    out[2 * pc.n + 2] = b.num_witness; out[2 * pc.n + 3] = b.num_instance;
    return b.bytes;
}
}

namespace {
int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
        }                                               \
    } while (0)

// every piece written to its last byte inside an allocation of exactly `bytes`, then read back
void fill_and_check(const Pieces &pc, unsigned char *mem, size_t bytes, const char *what)
{
    for (int i = 0; i < pc.n; i++) {
        CHECK(((uintptr_t)pc.p[i] & 15) == 0, "%s: piece %d is not 16-byte aligned", what, i);
        CHECK((const unsigned char *)pc.p[i] + pc.len[i] <= mem + bytes, "%s: piece %d ends beyond the workspace", what, i);
        memset((void *)pc.p[i], i + 1, pc.len[i]);
    }
    for (int i = 0; i < pc.n; i++)
        for (size_t j = 0; j < pc.len[i]; j++)
            if (((const unsigned char *)pc.p[i])[j] != i + 1) { CHECK(false, "%s: piece %d overlaps another at byte %zu", what, i, j); break; }
}

std::vector<uint8_t> pattern(size_t bytes, unsigned seed)
{
    std::vector<uint8_t> v(bytes);
    uint32_t x = 2463534242u + seed;
    for (uint8_t &b : v) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        b = (uint8_t)(x >> 11);
    }
    return v;
}

// one aggregate through StagedAggregate: every source exactly as long as a caller's, the stage exactly as long as reported
void stage(const std::vector<int> &logn, const std::vector<size_t> &lengths, bool nonces, bool with_rs, uint64_t first_off)
{
    const size_t count = logn.size();
    size_t c9 = 0, c10 = 0, pk_total = 0, sig_total = 0;
    for (int l : logn) {
        (l == 9 ? c9 : c10)++;
        pk_total += FRW_PK_LEN(l);
        sig_total += FRW_SIG_LEN(l);
    }
    std::vector<uint64_t> off(count + 1, first_off);
    for (size_t i = 0; i < count; i++) off[i + 1] = off[i] + lengths[i];
    const size_t second_total = nonces ? count * FRW_NONCE_LEN : sig_total, msg_total = (size_t)(off[count] - off[0]);
    const std::vector<uint8_t> pk = pattern(pk_total, 1), second = pattern(second_total, 2), blob = pattern((size_t)off[count], 3);
    const std::vector<uint8_t> rs_bytes = pattern(64, 4);
    uint64_t rs[8];
    memcpy(rs, rs_bytes.data(), 64);
    CHECK(frw::aggregate_pk_bytes(c9, c10) == pk_total && frw::aggregate_sig_bytes(c9, c10) == sig_total, "totals of %zu statements", count);
    const frw::StagedAggregate in(c9, c10, nonces, pk.data(), second.data(), blob.data(), off.data(), with_rs ? rs : nullptr);
    CHECK(in.pk_total == pk_total && in.second_total == second_total && in.msg_total == msg_total && in.count == count, "%zu statements", count);
    CHECK(in.o_pk == 0 && in.o_second % 256 == 0 && in.o_msgs % 256 == 0 && in.o_off % 256 == 0 && in.o_rs % 256 == 0 && in.bytes % 256 == 0,
          "%zu statements: 256-byte aligned pieces", count);
    CHECK(in.o_second >= pk_total && in.o_msgs >= in.o_second + second_total && in.o_off >= in.o_msgs + msg_total &&
          in.o_rs >= in.o_off + (count + 1) * 8 && in.bytes >= in.o_rs + (with_rs ? 64 : 0), "%zu statements: pieces in order", count);
    uint8_t *st = (uint8_t *)malloc(in.bytes);
    if (!st) exit(2);
    memset(st, 0xEE, in.bytes);
    in.fill(st);
    CHECK(memcmp(in.d_pk(st), pk.data(), pk_total) == 0, "pk bytes");
    CHECK(memcmp(in.d_second(st), second.data(), second_total) == 0, "second piece");
    CHECK(msg_total == 0 || memcmp(in.d_msgs(st), blob.data() + first_off, msg_total) == 0, "messages");
    const uint64_t *o = in.d_off(st);
    for (size_t i = 0; i <= count; i++) CHECK(o[i] == off[i] - off[0], "offset %zu", i);
    if (with_rs) CHECK(memcmp(in.d_rs(st), rs_bytes.data(), 64) == 0, "r, s");
    // every statement's bytes are where the routing function says
    size_t k[2] = {0, 0}, pk_at = 0, sig_at = 0;
    for (size_t s = 0; s < count; s++) {
        const int g = logn[s] - 9;
        const frw::AggRoute r = frw::aggregate_route(g, k[g], s);
        CHECK(r.pk_off == pk_at && r.sig_off == sig_at && r.nonce_off == s * 40, "statement %zu", s);
        CHECK(memcmp(in.d_pk(st) + r.pk_off, pk.data() + pk_at, FRW_PK_LEN(logn[s])) == 0, "statement %zu: its key", s);
        k[g]++;
        pk_at += FRW_PK_LEN(logn[s]);
        sig_at += FRW_SIG_LEN(logn[s]);
    }
    // nothing between the pieces was touched
    const size_t ends[5] = {pk_total, in.o_second + second_total, in.o_msgs + msg_total, in.o_off + (count + 1) * 8, with_rs ? in.o_rs + 64 : in.bytes};
    const size_t next[5] = {in.o_second, in.o_msgs, in.o_off, with_rs ? in.o_rs : in.bytes, in.bytes};
    for (int q = 0; q < 5; q++)
        for (size_t j = ends[q]; j < next[q]; j++)
            if (st[j] != 0xEE) { CHECK(false, "byte %zu after piece %d was written", j, q); break; }
    free(st);
}
}  // namespace

int main()
{
    const size_t counts[][2] = {{1, 0}, {0, 1}, {2, 1}, {1, 2}, {4, 3}, {290, 10}, {0, 0}};
    for (const auto &c : counts) {
        {
            const size_t bytes = frw::aggregate_screen_layout(nullptr, c[0], c[1]).bytes;
            unsigned char *mem = (unsigned char *)aligned_alloc(256, (bytes + 255) / 256 * 256);
            if (!mem) return 2;
            Pieces pc;
            screen_pieces(frw::aggregate_screen_layout(mem, c[0], c[1]), c[0], c[1], pc);
            fill_and_check(pc, mem, bytes, "screen");
            free(mem);
            printf("screen %zu + %zu: %zu bytes, %d pieces disjoint\n", c[0], c[1], bytes, pc.n);
        }
        if (c[0] + c[1] <= 3) {                                  // (the prover's holds 2.5 | 5 MB of witness a statement, twice)
            const size_t g16 = 4096 + 256, bytes = frw::aggregate_prove_layout(nullptr, c[0], c[1], g16).bytes;
            unsigned char *mem = (unsigned char *)aligned_alloc(256, (bytes + 255) / 256 * 256);
            if (!mem) return 2;
            const frw::AggregateProveBufs b = frw::aggregate_prove_layout(mem, c[0], c[1], g16);
            Pieces pc;
            prove_pieces(b, c[0], c[1], pc);
            pc.add(b.groth16_ws, b.groth16_bytes);
            fill_and_check(pc, mem, bytes, "prove");
            CHECK(((uintptr_t)b.witness & 255) == 0 && ((uintptr_t)b.groth16_ws & 255) == 0 && ((uintptr_t)b.set_witness[0] & 255) == 0 &&
                  ((uintptr_t)b.set_witness[1] & 255) == 0, "witnesses / prover workspace 256-byte aligned");
            free(mem);
            printf("prove %zu + %zu: %zu bytes, %d pieces disjoint\n", c[0], c[1], bytes, pc.n);
        }
    }
    int staged = 0;
    const std::vector<std::vector<int>> lists = {{9}, {10}, {9, 10, 9}, {10, 9, 10}, {10, 9, 9, 10, 9, 10, 9}};
    for (const std::vector<int> &logn : lists) {
        std::vector<size_t> lengths(logn.size());
        const size_t some[7] = {0, 95, 96, 97, 137, 1, 0};
        for (size_t i = 0; i < logn.size(); i++) lengths[i] = some[i % 7];
        stage(logn, lengths, false, false, 0);                               // verification's
        stage(logn, lengths, true, false, 3);                                // the statement's: nonces; the first offset is not 0
        stage(logn, lengths, false, true, 0);                                // the prover's: with r, s
        stage(logn, std::vector<size_t>(logn.size(), 0), false, true, 11);   // no message byte at all
        staged += 4;
    }
    if (failures) {
        printf("aggregate_bytes: %d check(s) failed\n", failures);
        return 1;
    }
    printf("%d aggregates staged\n", staged);
    printf("aggregate_bytes: clean\n");
    return 0;
}
