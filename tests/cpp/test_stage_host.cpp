// Test-only: the host side of the bytes paths (falcon-r1cs_amd/csrc/frw_stage.h), as a program of its own that
// tests/test_stage_host.py builds with -fsanitize=address,undefined and runs.
//   StagedInputs: every pass of a batch is filled into a heap buffer of exactly the size the layout reports; every staged piece must
//   equal the plain slice of its source, every rebased offset list start at 0 and end at the pass's message bytes, the longest pass be
//   the longest pass -- and the sanitizers see every byte written or read outside the buffer or the sources.
//   circuit_shape: for every (circuit, logn) the counts frw_layout* report (the library's, linked in: nothing here needs a device).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frw_stage.h"

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

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

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

// one batch through StagedInputs in passes of `chunk`; `with_msgs` false: msgs == NULL (every length must be 0 then)
void run(int logn, const std::vector<size_t> &lengths, size_t chunk, size_t second_len, bool with_rs, bool with_msgs, uint64_t first_off)
{
    const size_t batch = lengths.size(), pk_len = FRW_PK_LEN(logn);
    std::vector<uint64_t> off(batch + 1, first_off);
    for (size_t i = 0; i < batch; i++) off[i + 1] = off[i] + lengths[i];
    // exactly as long as the callers' arrays are: one byte more read from any of them trips the sanitizer
    const std::vector<uint8_t> pk = pattern(batch * pk_len, 1), second = pattern(batch * second_len, 2), blob = pattern((size_t)off[batch], 3);
    const std::vector<uint8_t> rs_bytes = pattern(batch * 64, 4);
    std::vector<uint64_t> rs(batch * 8);
    memcpy(rs.data(), rs_bytes.data(), batch * 64);
    const uint8_t *msgs = with_msgs ? blob.data() : nullptr;
    CHECK(frw::message_offsets_ok(msgs, off.data(), batch), "batch %zu chunk %zu", batch, chunk);
    const frw::StagedInputs in(logn, batch, chunk, pk.data(), second.data(), second_len, msgs, off.data(), with_rs ? rs.data() : nullptr);

    size_t longest = 1;
    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t hi = lo + chunk < batch ? lo + chunk : batch;
        if ((size_t)(off[hi] - off[lo]) > longest) longest = (size_t)(off[hi] - off[lo]);
    }
    CHECK(in.max_msg == longest, "longest pass %zu, reported %zu", longest, in.max_msg);
    // the offsets the four callers computed before there was one type for them
    const size_t o_second = up256(chunk * pk_len), o_msgs = o_second + up256(chunk * second_len), o_off = o_msgs + up256(longest);
    const size_t o_rs = o_off + up256((chunk + 1) * 8), bytes = o_rs + (with_rs ? up256(chunk * 64) : 0);
    CHECK(in.o_pk == 0 && in.o_second == o_second && in.o_msgs == o_msgs && in.o_off == o_off && in.bytes == bytes, "batch %zu chunk %zu", batch, chunk);
    CHECK(!with_rs || in.o_rs == o_rs, "batch %zu chunk %zu", batch, chunk);

    for (size_t lo = 0; lo < batch; lo += chunk) {
        const size_t cnt = lo + chunk < batch ? chunk : batch - lo, msg_bytes = (size_t)(off[lo + cnt] - off[lo]);
        uint8_t *stage = (uint8_t *)malloc(in.bytes);
        if (!stage) exit(2);
        memset(stage, 0xEE, in.bytes);
        in.fill(stage, lo, cnt);
        CHECK(in.msg_bytes(lo, cnt) == msg_bytes, "pass at %zu", lo);
        CHECK(in.d_pk(stage) == stage + in.o_pk && in.d_second(stage) == stage + in.o_second && in.d_msgs(stage) == stage + in.o_msgs &&
              (const uint8_t *)in.d_off(stage) == stage + in.o_off && (const uint8_t *)in.d_rs(stage) == stage + in.o_rs, "pass at %zu", lo);
        CHECK(memcmp(in.d_pk(stage), pk.data() + lo * pk_len, cnt * pk_len) == 0, "pk bytes of the pass at %zu", lo);
        CHECK(memcmp(in.d_second(stage), second.data() + lo * second_len, cnt * second_len) == 0, "second piece of the pass at %zu", lo);
        CHECK(msg_bytes == 0 || memcmp(in.d_msgs(stage), blob.data() + (size_t)off[lo], msg_bytes) == 0, "messages of the pass at %zu", lo);
        const uint64_t *o = in.d_off(stage);
        CHECK(o[0] == 0 && o[cnt] == msg_bytes, "offsets of the pass at %zu: %llu .. %llu", lo, (unsigned long long)o[0], (unsigned long long)o[cnt]);
        for (size_t i = 0; i <= cnt; i++) CHECK(o[i] == off[lo + i] - off[lo], "offset %zu of the pass at %zu", i, lo);
        if (with_rs) CHECK(memcmp(in.d_rs(stage), rs_bytes.data() + lo * 64, cnt * 64) == 0, "r, s of the pass at %zu", lo);
        // nothing between the pieces was touched
        const size_t ends[5] = {cnt * pk_len, in.o_second + cnt * second_len, in.o_msgs + msg_bytes, in.o_off + (cnt + 1) * 8,
                                with_rs ? in.o_rs + cnt * 64 : in.bytes};
        const size_t next[5] = {in.o_second, in.o_msgs, in.o_off, with_rs ? in.o_rs : in.bytes, in.bytes};
        for (int k = 0; k < 5; k++)
            for (size_t j = ends[k]; j < next[k]; j++)
                if (stage[j] != 0xEE) { CHECK(false, "byte %zu after piece %d of the pass at %zu was written", j, k, lo); break; }
        free(stage);
    }
}

void shapes()
{
    for (int logn = 9; logn <= 10; logn++) {
        frw_layout_t a;
        frw_layout_dual_t b;
        frw_layout_schoolbook_t c;
        CHECK(frw_layout(logn, &a) == FRW_OK && frw_layout_dual(logn, &b) == FRW_OK && frw_layout_schoolbook(logn, &c) == FRW_OK, "logn %d", logn);
        const int64_t want[3][4] = {{a.n, a.num_instance, a.num_witness, a.num_constraints},
                                    {b.n, b.num_instance, b.num_witness, b.num_constraints},
                                    {c.n, c.num_instance, c.num_witness, c.num_constraints}};
        const int sum[3] = {a.seg_off[FRW_NUM_SEGMENTS - 1] + a.seg_len[FRW_NUM_SEGMENTS - 1],
                            b.seg_off[FRW_NUM_SEGMENTS_DUAL - 1] + b.seg_len[FRW_NUM_SEGMENTS_DUAL - 1],
                            c.seg_off[FRW_NUM_SEGMENTS_SCHOOLBOOK - 1] + c.seg_len[FRW_NUM_SEGMENTS_SCHOOLBOOK - 1]};
        for (int circuit = 0; circuit < 3; circuit++) {
            const frw::CircuitShape s = frw::circuit_shape(circuit, logn);
            CHECK(frw::known_circuit(circuit), "circuit %d", circuit);
            CHECK((int64_t)s.n == want[circuit][0] && (int64_t)s.num_instance == want[circuit][1] && (int64_t)s.num_witness == want[circuit][2] &&
                  (int64_t)s.num_constraints == want[circuit][3], "circuit %d logn %d", circuit, logn);
            CHECK((size_t)sum[circuit] == s.num_witness, "the segments of circuit %d logn %d add up to %d", circuit, logn, sum[circuit]);
            CHECK(s.nb == (logn == 9 ? 50u : 52u), "circuit %d logn %d", circuit, logn);
        }
        CHECK(frw::circuit_shape(3, logn).num_witness == 0 && frw::circuit_shape(-1, logn).n == 0, "an unknown circuit has no shape");
    }
    CHECK(!frw::known_circuit(-1) && !frw::known_circuit(3), "unknown circuits");
}

void offsets()
{
    const uint8_t byte = 0;
    const uint64_t up[4] = {3, 3, 8, 8}, down[4] = {0, 8, 4, 9}, flat[4] = {5, 5, 5, 5};
    CHECK(frw::message_offsets_ok(&byte, up, 3) && frw::message_offsets_ok(&byte, flat, 3), "non-decreasing offsets");
    CHECK(!frw::message_offsets_ok(&byte, down, 3) && !frw::message_offsets_ok(&byte, down, 2), "decreasing offsets");
    CHECK(frw::message_offsets_ok(&byte, down, 1), "the first two offsets alone");
    CHECK(!frw::message_offsets_ok(nullptr, up, 3) && frw::message_offsets_ok(nullptr, flat, 3), "msgs == NULL only without message bytes");
    CHECK(frw::message_offsets_ok(nullptr, up, 1) && frw::message_offsets_ok(nullptr, up, 0), "msgs == NULL: an empty first message, an empty batch");
}
}  // namespace

int main()
{
    const std::vector<size_t> five = {0, 1, 135, 136, 137};                    // either side of SHAKE256's rate (136), the empty message
    const std::vector<size_t> seven = {0, 0, 0, 137, 136, 1, 135};             // chunks of 1, 2 and 3 have an all-empty pass
    int runs = 0;
    for (const std::vector<size_t> *lengths : {&five, &seven})
        for (size_t chunk : {1, 2, 3, 7}) {
            if (chunk > lengths->size()) chunk = lengths->size();              // (a chunk is never longer than its batch)
            run(9, *lengths, chunk, FRW_NONCE_LEN, false, true, 0);            // the statement's: nonces
            run(9, *lengths, chunk, 666, false, true, 3);                      // verification's: signatures; the first offset is not 0
            run(10, *lengths, chunk, 1280, true, true, 0);                     // the prover's: with r, s
            run(9, std::vector<size_t>(lengths->size(), 0), chunk, 666, true, false, 11);     // msgs absent, every length 0
            runs += 4;
        }
    shapes();
    offsets();
    if (failures) {
        printf("stage_host: %d check(s) failed\n", failures);
        return 1;
    }
    printf("%d batches staged pass by pass, 6 circuit shapes\n", runs);
    printf("stage_host: clean\n");
    return 0;
}
