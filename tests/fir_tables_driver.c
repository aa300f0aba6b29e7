/* The tables that the frequency-domain FIR forms upload, read back byte for byte over the stubbed device shim (the stub of
 * tests/test_host_sanitizers.py: device memory is host memory, and llzs_table_capture(1) / llzs_table_captured give every uploaded
 * table's address and size), under AddressSanitizer + UBSan.  Only the public API is called.  What the host layer promises and
 * this driver holds it to, none of it a matter of libm:
 *   * equal taps give equal float32 entries: a LLZ_FIR_ALGO_PARTITIONED handle's spectra are every channel's rows of a
 *     llz_fir_pbank_mc_init handle given the same taps in each of 3 channels (1, 513, 2049, 8193 taps: 1024, 1024 with two
 *     partitions, 2048 and 8192 points); a llz_fir_stream_mc handle with rows = 1 has the rows of a rows = channels handle and
 *     of every path of a 2-output x 3-input llz_fir_matrix_mc handle ((block, taps) = (64, 1), (64, 65), (512, 513));
 *   * set_taps on every per-row form (bank overlap-save, partitioned bank, stream with rows = channels, matrix): the taps of the
 *     init again change no byte of any table; new taps on one middle row give the tables of a fresh init and touch no other row;
 *   * more rows than one 8 MiB staging chunk holds (9 rows of 131073 taps at block 128): ceil(rows / rows per chunk) uploads, one
 *     behind the other, and every row equal to the row built alone.
 * With --dump it also prints the size and an FNV-1a-64 hash of every captured table, in upload order, of these cases and of the
 * overlap-save forms: the figures depend on libm, so they serve to compare two builds on one machine, not as a test. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "llz_shim.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static int g_dump;
static unsigned g_seed = 13579u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

static float *random_taps(size_t count)
{
    float *t = malloc(sizeof(float) * count);
    for (size_t i = 0; t && i < count; i++) t[i] = rnd();
    return t;
}

/* `copies` times the same T taps */
static float *repeated_taps(const float *taps, int T, int copies)
{
    float *t = malloc(sizeof(float) * (size_t)copies * (size_t)T);
    for (int c = 0; t && c < copies; c++) memcpy(t + (size_t)c * (size_t)T, taps, sizeof(float) * (size_t)T);
    return t;
}

/* the tables of one init, in upload order; --dump prints those of a labelled one */
typedef struct {
    int n;
    llzs_table_ref t[LLZS_MAX_TABLES];
} tables_t;

static void capture_begin(void) { llzs_table_capture(1); }

static void capture_end(const char *label, tables_t *c)
{
    c->n = llzs_table_captured(c->t, LLZS_MAX_TABLES);
    llzs_table_capture(0);
    for (int i = 0; g_dump && label && i < c->n && i < LLZS_MAX_TABLES; i++) {
        unsigned long long h = 14695981039346656037ull;
        const unsigned char *p = c->t[i].dev;
        for (size_t b = 0; b < c->t[i].bytes; b++) h = (h ^ p[b]) * 1099511628211ull;
        printf("%s table %d: %zu B fnv1a64 %016llx\n", label, i, c->t[i].bytes, h);
    }
}

static const unsigned char *table(const tables_t *c, int i) { return c->t[i].dev; }

/* ---- equal taps, equal entries: the shared partitioned handle against the partitioned bank ---- */
static int shared_against_bank(int T, int N)
{
    enum { CH = 3, FRAME = 256 };
    const int P = (T + N / 2 - 1) / (N / 2);
    const size_t row = sizeof(float) * 2 * (size_t)P * (size_t)N;
    char label[64];
    tables_t one, bank;
    float *taps = random_taps((size_t)T), *taps3 = taps ? repeated_taps(taps, T, CH) : NULL;
    CHECK(taps && taps3);
    snprintf(label, sizeof label, "partitioned T=%d", T);
    capture_begin();
    unsigned long h1 = llz_fir_filter_mc_init(CH, FRAME, taps, T, LLZ_FIR_ALGO_PARTITIONED);
    capture_end(label, &one);
    CHECK(h1 != BAD);
    snprintf(label, sizeof label, "pbank T=%d", T);
    capture_begin();
    unsigned long h3 = llz_fir_pbank_mc_init(CH, FRAME, taps3, T);
    capture_end(label, &bank);
    CHECK(h3 != BAD);
    /* shared: the padded taps, the spectra, the twiddles; bank: the spectra, the twiddles */
    CHECK(one.n == 3 && bank.n == 2);
    CHECK(one.t[1].bytes == row && bank.t[0].bytes == CH * row);
    for (int c = 0; c < CH; c++) CHECK(memcmp(table(&bank, 0) + (size_t)c * row, table(&one, 1), row) == 0);
    CHECK(one.t[2].bytes == sizeof(float) * (size_t)N && bank.t[1].bytes == one.t[2].bytes);
    CHECK(memcmp(table(&bank, 1), table(&one, 2), one.t[2].bytes) == 0);
    llz_fir_filter_mc_uninit(h1);
    llz_fir_bank_mc_uninit(h3);
    free(taps); free(taps3);
    printf("partitioned T=%d N=%d P=%d: shared spectra = each of %d bank rows\n", T, N, P, CH);
    return 0;
}

/* ---- the stream handle with one tap set against a row per channel and against the paths of a matrix ---- */
static int stream_against_rows_and_matrix(int B, int T)
{
    enum { CH = 3, OUTS = 2 };
    const int P = (T + B - 1) / B;
    const size_t row = sizeof(float) * 2 * (size_t)P * (size_t)B, tw = sizeof(float) * 2 * ((size_t)B / 2 + (size_t)B);
    char label[64];
    tables_t one, rows, mx;
    float *taps = random_taps((size_t)T), *taps6 = taps ? repeated_taps(taps, T, OUTS * CH) : NULL;
    CHECK(taps && taps6);
    snprintf(label, sizeof label, "stream B=%d T=%d rows=1", B, T);
    capture_begin();
    unsigned long h1 = llz_fir_stream_mc_init(CH, B, B, taps, 1, T);
    capture_end(label, &one);
    CHECK(h1 != BAD);
    snprintf(label, sizeof label, "stream B=%d T=%d rows=%d", B, T, CH);
    capture_begin();
    unsigned long h3 = llz_fir_stream_mc_init(CH, B, B, taps6, CH, T);
    capture_end(label, &rows);
    CHECK(h3 != BAD);
    snprintf(label, sizeof label, "matrix B=%d T=%d %dx%d", B, T, OUTS, CH);
    capture_begin();
    unsigned long hx = llz_fir_matrix_mc_init(CH, OUTS, B, B, taps6, T);
    capture_end(label, &mx);
    CHECK(hx != BAD);
    /* stream: the spectra, the twiddles; matrix: the spectra of every output's paths, the connection table, the twiddles */
    CHECK(one.n == 2 && rows.n == 2 && mx.n == OUTS + 2);
    CHECK(one.t[0].bytes == row && rows.t[0].bytes == CH * row);
    for (int c = 0; c < CH; c++) CHECK(memcmp(table(&rows, 0) + (size_t)c * row, table(&one, 0), row) == 0);
    for (int o = 0; o < OUTS; o++) {
        CHECK(mx.t[o].bytes == CH * row);
        for (int c = 0; c < CH; c++) CHECK(memcmp(table(&mx, o) + (size_t)c * row, table(&one, 0), row) == 0);
    }
    CHECK(one.t[1].bytes == tw && rows.t[1].bytes == tw && mx.t[OUTS + 1].bytes == tw);
    CHECK(memcmp(table(&rows, 1), table(&one, 1), tw) == 0 && memcmp(table(&mx, OUTS + 1), table(&one, 1), tw) == 0);
    llz_fir_stream_mc_uninit(h1);
    llz_fir_stream_mc_uninit(h3);
    llz_fir_matrix_mc_uninit(hx);
    free(taps); free(taps6);
    printf("stream B=%d T=%d P=%d: one tap set = each of %d rows = each of %d x %d matrix paths\n", B, T, P, CH, OUTS, CH);
    return 0;
}

/* ---- set_taps on the per-row forms ---- */
enum { BANK_OLS, PBANK, STREAM_ROWS, MATRIX, FORMS };
enum { M_OUTS = 2, M_INS = 3 };

/* a form's shape here, and which tap rows each of its tables holds (count 0: none, the table never changes) */
static const struct form {
    const char *name;
    int rows, T, block, middle, ntables;
    struct { int first, count; } held[4];
} FORM[FORMS] = {
    {"bank overlap-save", 3, 257, 0, 1, 3, {{0, 0}, {0, 3}, {0, 3}}},         /* twiddles, padded taps, spectra */
    {"partitioned bank", 3, 513, 0, 1, 2, {{0, 3}, {0, 0}}},                  /* spectra, twiddles */
    {"stream rows", 3, 65, 64, 1, 2, {{0, 3}, {0, 0}}},                       /* spectra, twiddles */
    /* the spectra of output 0's and output 1's paths, a connection byte per path (every path here is connected), twiddles */
    {"matrix", M_OUTS * M_INS, 65, 64, 4, 4, {{0, 3}, {3, 3}, {0, 6}, {0, 0}}},
};

static unsigned long form_init(int form, const float *taps)
{
    const struct form *F = &FORM[form];
    switch (form) {
    case BANK_OLS: return llz_fir_bank_mc_init(F->rows, 256, taps, F->T, LLZ_FIR_ALGO_OVERLAP_SAVE);
    case PBANK: return llz_fir_pbank_mc_init(F->rows, 256, taps, F->T);
    case STREAM_ROWS: return llz_fir_stream_mc_init(F->rows, F->block, F->block, taps, F->rows, F->T);
    default: return llz_fir_matrix_mc_init(M_INS, M_OUTS, F->block, F->block, taps, F->T);
    }
}

static int form_set_taps(int form, unsigned long h, int first, int count, const float *taps)
{
    switch (form) {
    case BANK_OLS: case PBANK: return llz_fir_bank_mc_set_taps(h, first, count, taps);
    case STREAM_ROWS: return llz_fir_stream_mc_set_taps(h, first, count, taps);
    default:
        /* whole outputs, or some paths of one output */
        if (first % M_INS == 0 && count % M_INS == 0)
            return llz_fir_matrix_mc_set_taps(h, first / M_INS, count / M_INS, 0, M_INS, taps);
        return llz_fir_matrix_mc_set_taps(h, first / M_INS, 1, first % M_INS, count, taps);
    }
}

static void form_uninit(int form, unsigned long h)
{
    if (form == BANK_OLS || form == PBANK) llz_fir_bank_mc_uninit(h);
    else if (form == STREAM_ROWS) llz_fir_stream_mc_uninit(h);
    else llz_fir_matrix_mc_uninit(h);
}

static int set_taps_keeps_and_replaces(int form)
{
    const struct form *F = &FORM[form];
    const size_t T = (size_t)F->T;
    char label[64];
    tables_t now, fresh;
    unsigned char *was[4] = {NULL, NULL, NULL, NULL};
    float *taps = random_taps((size_t)F->rows * T), *other = random_taps(T);
    CHECK(taps && other);
    snprintf(label, sizeof label, "%s T=%d", F->name, F->T);
    capture_begin();
    unsigned long h = form_init(form, taps);
    capture_end(label, &now);
    CHECK(h != BAD && now.n == F->ntables);
    for (int i = 0; i < now.n; i++) {
        CHECK(was[i] = malloc(now.t[i].bytes));
        memcpy(was[i], table(&now, i), now.t[i].bytes);
    }
    /* the taps it was initialised with: no byte of any table changes */
    CHECK(form_set_taps(form, h, 0, F->rows, taps) == 0);
    for (int i = 0; i < now.n; i++) CHECK(memcmp(table(&now, i), was[i], now.t[i].bytes) == 0);
    /* new taps on the middle row: the tables of a fresh init with that row, and no byte outside the row has changed */
    CHECK(form_set_taps(form, h, F->middle, 1, other) == 0);
    memcpy(taps + (size_t)F->middle * T, other, sizeof(float) * T);
    capture_begin();
    unsigned long hf = form_init(form, taps);
    capture_end(NULL, &fresh);
    CHECK(hf != BAD && fresh.n == now.n);
    for (int i = 0; i < now.n; i++) {
        const size_t bytes = now.t[i].bytes;
        CHECK(fresh.t[i].bytes == bytes && memcmp(table(&now, i), table(&fresh, i), bytes) == 0);
        const int r = F->middle - F->held[i].first;
        if (r < 0 || r >= F->held[i].count) {
            CHECK(memcmp(table(&now, i), was[i], bytes) == 0);
            continue;
        }
        const size_t len = bytes / (size_t)F->held[i].count, off = (size_t)r * len;
        CHECK(memcmp(table(&now, i), was[i], off) == 0);
        CHECK(memcmp(table(&now, i) + off + len, was[i] + off + len, bytes - off - len) == 0);
        /* the row itself has changed, but for a connection byte: both tap rows are connected */
        CHECK(len == 1 || memcmp(table(&now, i) + off, was[i] + off, len) != 0);
    }
    form_uninit(form, h);
    form_uninit(form, hf);
    for (int i = 0; i < 4; i++) free(was[i]);
    free(taps); free(other);
    printf("%s T=%d: set_taps keeps equal taps' tables and replaces row %d alone\n", F->name, F->T, F->middle);
    return 0;
}

/* ---- more rows than one staging chunk holds ---- */
static int chunked_rows(void)
{
    enum { B = 128, T = 131073, ROWS = 9 };
    const int P = (T + B - 1) / B;
    const size_t row = sizeof(float) * 2 * (size_t)P * (size_t)B, per_chunk = ((size_t)8 << 20) / row;
    const int uploads = (int)((ROWS + per_chunk - 1) / per_chunk);
    tables_t all, one;
    float *taps = random_taps((size_t)ROWS * T);
    CHECK(taps && per_chunk >= 1 && uploads > 1);
    capture_begin();
    unsigned long h = llz_fir_stream_mc_init(ROWS, B, B, taps, ROWS, T);
    capture_end("stream B=128 T=131073 rows=9", &all);
    CHECK(h != BAD && all.n == uploads + 1);                       /* the chunks, then the twiddles */
    for (int u = 0; u < uploads; u++) {
        const size_t rows = u + 1 < uploads ? per_chunk : ROWS - (size_t)u * per_chunk;
        CHECK(all.t[u].bytes == rows * row && table(&all, u) == table(&all, 0) + (size_t)u * per_chunk * row);
    }
    for (int r = 0; r < ROWS; r++) {
        capture_begin();
        unsigned long h1 = llz_fir_stream_mc_init(1, B, B, taps + (size_t)r * T, 1, T);
        capture_end(NULL, &one);
        CHECK(h1 != BAD && one.n == 2 && one.t[0].bytes == row);
        CHECK(memcmp(table(&all, 0) + (size_t)r * row, table(&one, 0), row) == 0);
        llz_fir_stream_mc_uninit(h1);
    }
    llz_fir_stream_mc_uninit(h);
    free(taps);
    printf("stream B=%d T=%d: %d rows in %d uploads of at most %zu rows = the rows built alone\n", B, T, ROWS, uploads, per_chunk);
    return 0;
}

/* ---- --dump alone: the overlap-save forms, whose tables no other form shares ---- */
static int dump_overlap_save(void)
{
    static const int rung[4][2] = {{33, LLZ_FIR_ALGO_OVERLAP_SAVE}, {600, LLZ_FIR_ALGO_OVERLAP_SAVE_2048},
                                   {1100, LLZ_FIR_ALGO_OVERLAP_SAVE_4096}, {3100, LLZ_FIR_ALGO_OVERLAP_SAVE_8192}};
    char label[64];
    tables_t c;
    for (int i = 0; i < 4; i++) {
        float *taps = random_taps((size_t)rung[i][0]);
        CHECK(taps);
        snprintf(label, sizeof label, "overlap-save T=%d algo=%d", rung[i][0], rung[i][1]);
        capture_begin();
        unsigned long h = llz_fir_filter_mc_init(2, 256, taps, rung[i][0], rung[i][1]);
        capture_end(label, &c);
        CHECK(h != BAD && c.n >= 3);
        llz_fir_filter_mc_uninit(h);
        free(taps);
    }
    float *taps = random_taps(4 * 257);
    CHECK(taps);
    capture_begin();
    unsigned long h = llz_fir_bank_mc_init(4, 256, taps, 257, LLZ_FIR_ALGO_OVERLAP_SAVE);
    capture_end("bank overlap-save 4 x 257", &c);
    CHECK(h != BAD && c.n == 3);
    llz_fir_bank_mc_uninit(h);
    free(taps);
    return 0;
}

int main(int argc, char **argv)
{
    static const int part[4][2] = {{1, 1024}, {513, 1024}, {2049, 2048}, {8193, 8192}};
    static const int stream[3][2] = {{64, 1}, {64, 65}, {512, 513}};
    g_dump = argc > 1 && strcmp(argv[1], "--dump") == 0;
    for (int i = 0; i < 4; i++)
        if (shared_against_bank(part[i][0], part[i][1])) return 1;
    for (int i = 0; i < 3; i++)
        if (stream_against_rows_and_matrix(stream[i][0], stream[i][1])) return 1;
    for (int form = 0; form < FORMS; form++)
        if (set_taps_keeps_and_replaces(form)) return 1;
    if (chunked_rows()) return 1;
    if (g_dump && dump_overlap_save()) return 1;
    printf("FIR_TABLES_OK\n");
    return 0;
}
