// Stand-alone host check of the super-block walk's geometry (llzlab_amd/csrc/kernels/ols_superblock.h): the walk of
// k_fir_ols_chain_f32 replayed on SAMPLE INDICES instead of samples, through the header's own functions (windows, requests,
// clamped references, the assemble steps that move the carried rows).  A row of 32 samples is stood for by the index of its
// first sample; columns are looked at one by one only where a row touches an end of the channel.
//   usage: ols_superblock_driver n_lo n_hi keep      -> every n in [n_lo, n_hi], one channel, a single wave walking all units
// For each n: every output sample in [0, n) is stored exactly once; the eight rows in front of every stored row (its samples'
// 256 predecessors) are what the block assembled; no request leaves [-keep, n); no live super-block index reaches the total.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ols_superblock.h"

namespace {

struct cplx { long x, y; };
struct raw_t { long a[24], b[24]; };
constexpr long NOTHING = -(1L << 40);          // a row nobody requested

int n, keep;
long total;
std::vector<int> next_of;                      // next_of[start] = end of the stored range that starts there, or -1
std::vector<int> starts;
long fails = 0;

#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL n=%d keep=%d: ", n, keep); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// a requested row: first sample st of the channel row
long request_row(long st, bool live, bool whole)
{
    if (whole) {
        CHECK(live && st >= 0 && st + OLS_SB_ROW <= n, "unclamped request [%ld, +32) outside [0, %d)", st, n);
        return st;
    }
    if (live && st >= 0 && st + OLS_SB_ROW <= n) return st;         // inside: every column reads its own sample
    for (int col = 0; col < OLS_SB_ROW; col++) {
        const ols_sb_ref r = ols_sb_sample((int)st + col, n, live);
        CHECK(r.addr >= 0 && r.addr < n, "request address %d outside [0, %d)", r.addr, n);
        CHECK(r.use == (live && st + col < n), "sample %ld: used %d", st + col, (int)r.use);
        CHECK(!r.use || r.addr == st + col, "sample %ld read at %d", st + col, r.addr);
    }
    return live && st < n ? st : NOTHING;
}

long halo_row(long st, bool live, bool has_hist)
{
    for (int col = 0; col < OLS_SB_ROW; col++) {
        const long idx = st + col;
        const ols_sb_href r = ols_sb_halo_sample((int)idx, n, keep, live, has_hist);
        if (r.src == OLS_SB_FROM_ROW) CHECK(r.addr == idx && idx >= 0 && idx < n, "halo sample %ld read at row[%d]", idx, r.addr);
        else if (r.src == OLS_SB_FROM_HIST) CHECK(has_hist && r.addr == keep + idx && r.addr >= 0 && r.addr < keep, "halo sample %ld read at hist[%d]", idx, r.addr);
        else CHECK(!live || idx >= n || idx < -keep || (idx < 0 && !has_hist), "halo sample %ld dropped", idx);
    }
    return live && st < n ? st : NOTHING;
}

struct half_t {
    long halo[16];
    raw_t raw;
};

template <int ROWS>
void load(half_t &h, long s, bool live, bool whole)
{
    for (int i = 0; i < ROWS; i++) {
        h.raw.a[i] = request_row(s + OLS_SB_ROW * i, live, whole);
        h.raw.b[i] = request_row(s + OLS_SB_REGION + OLS_SB_ROW * i, live, whole);
    }
}

void load_halo(half_t &h, long s, bool live)
{
    for (int i = 0; i < 8; i++) {
        h.halo[i] = halo_row(s - OLS_SB_HALO + OLS_SB_ROW * i, live, true);
        h.halo[8 + i] = halo_row(s - OLS_SB_HALO + OLS_SB_REGION + OLS_SB_ROW * i, live, false);
    }
}

// the block of job `job` of the super-block at s: rows >= carry are stored, and each stored row needs the 8 rows before it
void store(const cplx (&v)[32], long s, int job, bool live, bool whole)
{
    if (!live) return;
    const int carry = ols_sb_carry_rows(job);
    for (int sub = 0; sub < 2; sub++) {
        const long w = s + sub * OLS_SB_REGION + ols_sb_window(job);
        for (int r = carry; r < 32; r++) {
            const long st = w + OLS_SB_ROW * r;
            if (whole) CHECK(st >= 0 && st + OLS_SB_ROW <= n, "unbounded store [%ld, +32) outside [0, %d)", st, n);
            if (st >= n) continue;
            CHECK(st >= 0, "store at %ld", st);
            const int x = (int)(st - s - sub * OLS_SB_REGION);
            CHECK(ols_sb_job_of(x) == job && ols_sb_row_of(x) == r, "sample %d of a region: job %d row %d, stored by job %d row %d",
                  x, ols_sb_job_of(x), ols_sb_row_of(x), job, r);
            for (int q = r - 8; q <= r; q++) {
                const long have = sub ? v[q].y : v[q].x;
                CHECK(have == w + OLS_SB_ROW * q, "job %d sub %d row %d: holds row at %ld, wants %ld", job, sub, q, have, w + OLS_SB_ROW * q);
            }
            const int end = (int)(st + OLS_SB_ROW < n ? st + OLS_SB_ROW : n);
            CHECK(next_of[st] < 0, "sample %ld stored twice", st);
            next_of[st] = end;
            starts.push_back((int)st);
        }
    }
}

struct unit_t { bool live; long s; };
unit_t locate(long u)
{
    unit_t g;
    g.live = u < total;
    g.s = g.live ? (u % ols_sb_units_per_channel(n)) * (long)OLS_SB_UNIT : 0;
    if (g.live) CHECK(u < ols_sb_total(1, n) && g.s < n, "super-block %ld starts at %ld", u, g.s);
    return g;
}
bool whole_of(const unit_t (&u)[2])
{
    return u[0].live && u[1].live && ols_sb_whole((int)u[0].s, n) && ols_sb_whole((int)u[1].s, n);
}

void run_one()
{
    total = ols_sb_total(1, n);
    starts.clear();
    half_t H[2];
    unit_t cur[2] = {locate(0), locate(1)};
    for (int h = 0; h < 2; h++) {
        load_halo(H[h], cur[h].s, cur[h].live);
        load<24>(H[h], cur[h].s, cur[h].live, whole_of(cur));
    }
    for (long sp = 0; sp < total; sp += 2) {
        const unit_t nxt[2] = {locate(sp + 2), locate(sp + 3)};
        const bool whole = whole_of(cur);
        for (int jj = 0; jj < OLS_SB_FULL_JOBS; jj++) {
            for (int h = 0; h < 2; h++) {
                cplx v[32];
                ols_sb_assemble_full(v, H[h].halo, H[h].raw);
                const long sn = cur[h].s + ols_sb_request(jj + 1);
                if (jj + 1 < OLS_SB_FULL_JOBS) load<24>(H[h], sn, cur[h].live, whole);
                else load<16>(H[h], sn, cur[h].live, whole);
                store(v, cur[h].s, jj, cur[h].live, whole);
            }
        }
        for (int h = 0; h < 2; h++) {
            cplx v[32];
            ols_sb_assemble_short(v, H[h].halo, H[h].raw);
            load<24>(H[h], nxt[h].s, nxt[h].live, whole_of(nxt));
            load_halo(H[h], nxt[h].s, nxt[h].live);
            store(v, cur[h].s, OLS_SB_FULL_JOBS, cur[h].live, whole);
        }
        cur[0] = nxt[0];
        cur[1] = nxt[1];
    }
    // the stored ranges tile [0, n)
    int at = 0;
    size_t used = 0;
    while (at < n && next_of[at] > at) { at = next_of[at]; used++; }
    CHECK(at == n && used == starts.size(), "stored ranges reach %d of %d with %zu of %zu ranges", at, n, used, starts.size());
    for (int st : starts) next_of[st] = -1;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 4) { printf("usage: %s n_lo n_hi keep\n", argv[0]); return 2; }
    const int lo = atoi(argv[1]), hi = atoi(argv[2]);
    keep = atoi(argv[3]);
    if (lo < 1 || hi < lo || keep < 0 || keep > OLS_SB_HALO) { printf("bad arguments\n"); return 2; }
    static_assert(ols_sb_request(0) == 0 && ols_sb_request(OLS_SB_FULL_JOBS) + 16 * OLS_SB_ROW == OLS_SB_REGION, "a region is 10 full blocks and a short one");
    next_of.assign((size_t)hi + 1, -1);
    for (n = lo; n <= hi; n++) run_one();
    if (fails) { printf("OLS_SB_FAILED %ld checks\n", fails); return 1; }
    printf("OLS_SB_OK n=%d..%d keep=%d\n", lo, hi, keep);
    return 0;
}
