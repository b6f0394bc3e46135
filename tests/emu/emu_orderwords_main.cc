/*
 * Stand-alone sanitizer program of the order-words emulation — TEST TOOLING ONLY (tests/test_emu_order_words.py compiles it with g++
 * -fsanitize=address,undefined and runs it as a child process; nothing of it is loaded into Python).
 *
 *     emu_orderwords_main <batch file> <lean 0|1>
 *
 * The batch file is what the test writes from its logs: five u64 {n_logs, n_ops, n_changes, max_actors, env stride}, then the columns in the order of the reads
 * below.  Every block — the columns, the results, the index, the operand words, the order words and the tombstone words — is exactly as large as the host
 * library makes it (ptx_row_index_words 4-byte words of index and of order words, as many 8-byte operand words, ptx_row_bits_words words of each bitmap, a word
 * per log for each), so a word read or written outside its block is a report — and so is a read of the LDS lists that a reader of a standing log no longer
 * fills.  Four merges: the writer (lane order 0) and three readers (orders 1, 2, 0); a lean reader must not enter P3 for a log whose order word stands, a log
 * stands exactly if it gets through P3, and every result must equal the writer's.
 */
#include "emu_orderwords.cc"

#include <stdio.h>

#include <vector>

template <class T>
static T* read_col(FILE* f, size_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "short batch file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int lean = atoi(argv[2]);
    uint64_t h[5];
    if (fread(h, 8, 5, f) != 5) return 2;
    const size_t L = (size_t)h[0], R = (size_t)h[1], Cn = (size_t)h[2], stride = (size_t)h[4];
    ptx_batch b;
    memset(&b, 0, sizeof(b));
    b.n_logs = (uint32_t)L;
    b.n_ops = R;
    b.max_actors = (uint32_t)h[3];
    b.log_off = read_col<uint64_t>(f, L + 1);
    b.op_id = read_col<uint64_t>(f, R);
    b.ref_a = read_col<uint64_t>(f, R);
    b.ref_b = read_col<uint64_t>(f, R);
    b.payload = read_col<uint32_t>(f, R);
    b.action = read_col<uint8_t>(f, R);
    b.mark_type = read_col<uint8_t>(f, R);
    b.side_a = read_col<uint8_t>(f, R);
    b.side_b = read_col<uint8_t>(f, R);
    b.chg_off = read_col<uint64_t>(f, L + 1);
    b.chg_hdr = read_col<uint32_t>(f, Cn);
    b.chg_env = read_col<uint16_t>(f, Cn * stride);
    fclose(f);
    const size_t iw = (size_t)ptx_row_index_words(R, L), bw = (size_t)ptx_row_bits_words(R, L);
    uint32_t* index = (uint32_t*)malloc(iw * 4);
    uint32_t* bits = (uint32_t*)malloc(bw * 4);
    uint64_t* ops = (uint64_t*)malloc(iw * 8);
    uint32_t* rows_indexed = (uint32_t*)calloc(L ? L : 1, 4);
    uint32_t* stand = (uint32_t*)calloc(L ? L : 1, 4);
    memset(index, 0xEE, iw * 4); /* (the library never zeroes these three) */
    memset(bits, 0xEE, bw * 4);
    memset(ops, 0xEE, iw * 8);
    uint32_t* ow = (uint32_t*)malloc(iw * 4);
    uint32_t* ob = (uint32_t*)malloc(bw * 4);
    uint32_t* ostand = (uint32_t*)calloc(L ? L : 1, 4);
    memset(ow, 0xEE, iw * 4); /* (nor these two) */
    memset(ob, 0xEE, bw * 4);
    struct Out {
        std::vector<ptx_log_result> logs;
        std::vector<uint32_t> values;
        std::vector<ptx_cinterval> cints;
        std::vector<ptx_span> spans;
    } out[4];
    std::vector<unsigned long long> counts(3 * (L ? L : 1));
    unsigned long long reader_trees = 0;
    int bad = 0;
    for (int run = 0; run < 4; ++run) {
        Out& o = out[run];
        o.logs.assign(L ? L : 1, ptx_log_result());
        o.values.assign(R ? R : 1, 0u);
        o.cints.assign(R ? R : 1, ptx_cinterval());
        o.spans.assign(R ? R : 1, ptx_span());
        const int rc = ptx_emu_merge_orderwords(&b, o.logs.data(), o.values.data(), o.spans.data(), o.cints.data(), nullptr, nullptr, index, bits, rows_indexed, ops, stand, ow, ob,
                                                ostand, run == 0, 1, counts.data(), 160u * 1024u, run % 3, lean);
        if (rc) return 3;
        for (size_t l = 0; l < L; ++l) {
            const uint64_t N = b.log_off[l + 1] - b.log_off[l];
            const ptx_log_result &a = out[0].logs[l], &c = o.logs[l];
            if (memcmp(&a, &c, sizeof(a)) != 0) ++bad, fprintf(stderr, "run %d log %zu: result row differs from the writer's\n", run, l);
            if (a.status == PTX_OK && N && ostand[l] != N) ++bad, fprintf(stderr, "log %zu: passes, its order word %u != %llu\n", l, ostand[l], (unsigned long long)N);
            if (ostand[l] != 0 && ostand[l] != N) ++bad, fprintf(stderr, "log %zu: order word %u is neither 0 nor its row count\n", l, ostand[l]);
            if (run && ostand[l] == N && stand[l] == N) reader_trees += counts[3 * l];
            if (a.status == PTX_OK) {
                const uint64_t r0 = b.log_off[l];
                if (memcmp(&out[0].values[r0], &o.values[r0], (size_t)a.n_visible * 4) != 0) ++bad, fprintf(stderr, "run %d log %zu: values differ\n", run, l);
                if (memcmp(&out[0].spans[r0], &o.spans[r0], (size_t)a.n_spans * sizeof(ptx_span)) != 0) ++bad, fprintf(stderr, "run %d log %zu: spans differ\n", run, l);
            }
        }
    }
    size_t standing = 0;
    for (size_t l = 0; l < L; ++l) standing += ostand[l] != 0;
    printf("emu_orderwords_main: %zu logs, %zu rows, %llu tree passes by the readers of standing logs, %zu order words stand, %d disagreements\n", L, R, reader_trees, standing, bad);
    free(ow);
    free(ob);
    free(ostand);
    free(index);
    free(bits);
    free(ops);
    free(rows_indexed);
    free(stand);
    free((void*)b.log_off);
    free((void*)b.op_id);
    free((void*)b.ref_a);
    free((void*)b.ref_b);
    free((void*)b.payload);
    free((void*)b.action);
    free((void*)b.mark_type);
    free((void*)b.side_a);
    free((void*)b.side_b);
    free((void*)b.chg_off);
    free((void*)b.chg_hdr);
    free((void*)b.chg_env);
    return bad ? 1 : 0;
}
