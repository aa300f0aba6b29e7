"""The shim calls of the transform and analysis host layer (csrc/host: llz_fft_host.c, llz_mdct_host.c, llz_mdct_fixed_host.c,
llz_asmodel_host.c, llz_corr_host.c, llz_lpc_host.c, llz_lpc_filter_host.c, llz_spectral_host.c, llz_pcm_host.c, llz_util.c,
llz_tables.c), pinned as a trace.  The stand-alone driver tests/host_calls_driver.c runs every init and every call of these files,
with host buffers, with "device" buffers and (16-byte-rule handles) with device buffers 4 bytes off, against a shim stub that this
file generates from csrc/llz_shim.h, under AddressSanitizer + UBSan.  Unlike the stub of test_host_sanitizers.py this one keeps a
table of its allocations: llzs_is_device_ptr is 1 inside what llzs_malloc / llz_hip_malloc returned, and every llzs_* call writes
one line -- name, integer and size arguments, each pointer as "caller<k>+<offset>" or "lib<j>+<offset>", never an address, and a
64-bit FNV-1a hash of the bytes of every upload whose source is not a caller buffer, that is, of every table.  Pure queries
(llzs_is_device_ptr, llzs_tune, llzs_set_error) and llzs_free(NULL) write no line.

Per scenario the driver prints the name, the number of lines and the hash of the trace; host_calls_expected.txt holds those of the
commit before the host layer's consolidation (the same driver built against that commit's host/*.c in a git worktree), except for
the lines named below.  A handle's scenario is two lines, `<name>.init` and `<name>` (the calls and the uninit); `tables` is a hash
over the sizes and bytes of the uploaded tables alone.  The table hashes depend on libm's cos / sin, so the comparison holds between two builds on one
machine type; `host_calls --trace [scenario]` prints the full trace.

The driver then fails the k-th device allocation of every init and of every one-shot call, for every k the scenario reaches:
each must be refused (LLZ_BAD_HANDLE, or a negative code), and the program must end without a leak."""
import glob
import os
import re
import subprocess

import pytest

from tests.test_host_sanitizers import CSRC, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))

# The lines of host_calls_expected.txt that are NOT the earlier commit's (every other line is, verbatim):
#  * one-shot calls with a host buffer.  The one binder of llz_util.c synchronises the stream once before it frees what it
#    staged, and frees in declaration order: llz_autocorr_mc with only its output in host memory gains the llzs_sync (it leaned on
#    llzs_d2h's), llz_crosscorr_mc / llz_corr_cof_mc free x before y (the same calls otherwise).
CHANGED_CALLS = {"autocorr_mc_p5_dev_in_host_out", "crosscorr_mc_host", "crosscorr_mc_two_sided_host", "corr_cof_mc_host"}
#  * the inits that allocated all their tables before they uploaded any: each table is now uploaded as it is allocated (one
#    uploader, llz_host_upload).  The same allocations and the same uploads, in the same order among themselves: the `tables` hash
#    of these lines, and the calls behind these inits, are the earlier commit's.
CHANGED_INITS = ("mdct_origin", "mdct_fft", "mdct_fft4", "mdct_batch_32_", "analysis_mdct_8", "synthesis_mdct_8", "stft_mc_",
                 "mdct_frames_mc_", "csd_mc_")

STUB_HEAD = r'''
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_shim.h"
#include "llz_hip.h"
static char g_err[512];
void llzs_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
const char *llz_hip_last_error(void) { return g_err; }

enum { MAX_BLK = 4096 };
typedef struct { char *p; size_t n; int caller, id, device; } blk_t;
static blk_t g_blk[MAX_BLK];
static int g_bad_frees, g_nblk, g_nlib, g_ncaller, g_fail_at = -1, g_mallocs, g_print, g_lines, g_work;
static unsigned long long g_hash, g_thash;

static unsigned long long fnv(unsigned long long h, const void *p, size_t n)
{
    const unsigned char *b = p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
static void tr(int work, const char *fmt, ...)
{
    char line[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(line, sizeof line - 1, fmt, ap); va_end(ap);
    strcat(line, "\n");
    g_hash = fnv(g_hash, line, strlen(line));
    g_lines++; g_work += work;
    if (g_print) fputs(line, stdout);
}
static blk_t *find(const void *p)
{
    for (int i = 0; i < g_nblk; i++)
        if (g_blk[i].p && (const char *)p >= g_blk[i].p && (const char *)p < g_blk[i].p + (g_blk[i].n ? g_blk[i].n : 1)) return &g_blk[i];
    return NULL;
}
static const char *dp(const void *p)
{
    static char buf[16][48]; static int turn;
    char *s = buf[turn++ & 15];
    const blk_t *b = find(p);
    if (!p) return "null";
    if (!b) return "host";
    snprintf(s, 48, "%s%d+%zu", b->caller ? "caller" : "lib", b->id, (size_t)((const char *)p - b->p));
    return s;
}
static void *add(void *p, size_t n, int caller, int device)
{
    int i = 0;
    while (i < g_nblk && g_blk[i].p) i++;
    if (!p || i == MAX_BLK) { fprintf(stderr, "stub: out of memory or of blocks\n"); exit(3); }
    if (i == g_nblk) g_nblk++;
    g_blk[i].p = p; g_blk[i].n = n; g_blk[i].caller = caller; g_blk[i].device = device;
    g_blk[i].id = caller ? g_ncaller++ : g_nlib++;
    return p;
}
static void drop(void *p)
{
    blk_t *b = find(p);
    if (!b || b->p != p) { g_bad_frees++; return; }               /* freed twice, or never allocated here */
    b->p = NULL;
    free(p);
}
/* ---- the driver's side ---- */
void stub_begin(int print)
{
    for (int i = 0; i < g_nblk; i++)
        if (g_blk[i].p && !g_blk[i].caller) g_blk[i].p = NULL;      /* left behind by the scenario before: the leak check's at exit */
    g_hash = g_thash = 14695981039346656037ull; g_lines = g_work = 0; g_nlib = g_ncaller = 0; g_print = print; g_fail_at = -1; g_mallocs = 0; g_err[0] = 0;
}
/* the trace since stub_begin or the last cut: lines, their hash, and the hash of (size, bytes) of the tables uploaded; the numbering
 * of the allocations goes on */
void stub_cut(int *lines, unsigned long long *hash, unsigned long long *tables)
{
    *lines = g_lines; *hash = g_hash; *tables = g_thash;
    g_lines = 0; g_hash = g_thash = 14695981039346656037ull;
}
int stub_work(void) { return g_work; }                      /* lines written so far, llzs_device_* aside */
int stub_mallocs(void) { return g_mallocs; }
int stub_bad_frees(void) { return g_bad_frees; }
int stub_live(void) { int n = 0; for (int i = 0; i < g_nblk; i++) n += g_blk[i].p && !g_blk[i].caller; return n; }
void stub_fail_malloc(int k) { g_fail_at = k; g_mallocs = 0; }
void *stub_host(size_t n) { void *p = add(malloc(n ? n : 1), n, 1, 0); memset(p, 0x11, n); return p; }
void stub_host_free(void *p) { if (p) drop(p); }
void *llz_hip_malloc(size_t n) { return add(calloc(n ? n : 1, 1), n, 1, 1); }
void llz_hip_free(void *p) { if (p) drop(p); }
int llz_hip_device_count(void) { return 1; }
/* ---- the runtime of llz_shim.h ---- */
void *llzs_malloc(size_t n)
{
    if (g_mallocs++ == g_fail_at) { tr(1, "llzs_malloc bytes=%zu -> null", n); llzs_set_error("stub: allocation refused"); return NULL; }
    void *p = add(calloc(n ? n : 1, 1), n, 0, 1);
    tr(1, "llzs_malloc bytes=%zu -> %s", n, dp(p));
    return p;
}
void llzs_free(void *p) { if (!p) return; tr(1, "llzs_free %s", dp(p)); drop(p); }
static void up(const char *name, void *d, const void *s, size_t n, int st)
{
    const blk_t *b = find(s);
    if (b && b->caller) tr(1, "%s dst=%s src=%s bytes=%zu stream=%d", name, dp(d), dp(s), n, st);
    else {
        const unsigned long long h = fnv(14695981039346656037ull, s, n);
        tr(1, "%s dst=%s src=%s bytes=%zu stream=%d fnv=%016llx", name, dp(d), dp(s), n, st, h);
        g_thash = fnv(fnv(g_thash, &n, sizeof n), &h, sizeof h);
    }
    memcpy(d, s, n);
}
int llzs_h2d(void *d, const void *s, size_t n, void *st) { up("llzs_h2d", d, s, n, st != NULL); return 0; }
int llzs_h2d_table(void *d, const void *s, size_t n) { up("llzs_h2d_table", d, s, n, 0); return 0; }
int llzs_d2h(void *d, const void *s, size_t n, void *st) { tr(1, "llzs_d2h dst=%s src=%s bytes=%zu stream=%d", dp(d), dp(s), n, st != NULL); memcpy(d, s, n); return 0; }
int llzs_d2d(void *d, const void *s, size_t n, void *st) { tr(1, "llzs_d2d dst=%s src=%s bytes=%zu stream=%d", dp(d), dp(s), n, st != NULL); memmove(d, s, n); return 0; }
int llzs_memset(void *d, int v, size_t n, void *st) { tr(1, "llzs_memset dst=%s value=%d bytes=%zu stream=%d", dp(d), v, n, st != NULL); memset(d, v, n); return 0; }
int llzs_sync(void *st) { tr(1, "llzs_sync stream=%d", st != NULL); return 0; }
int llzs_is_device_ptr(const void *p) { const blk_t *b = find(p); return b ? b->device : 0; }
int llzs_tune(int id) { (void)id; return -1; }
int llzs_device_get(void) { tr(0, "llzs_device_get"); return 0; }
int llzs_device_enter(int d) { tr(0, "llzs_device_enter device=%d", d); return 0; }
void llzs_device_leave(int p) { tr(0, "llzs_device_leave previous=%d", p); }
int llzs_fft_large_twb_bytes(int size) { return 8 * size; }
int llzs_resample_mfma_f32_table_steps(int L, int M, int Q) { (void)L; (void)M; (void)Q; return 16; }
int llzs_resample_i16x_ksteps(int L, int M, int Q) { (void)L; (void)M; (void)Q; return 4; }
int llzs_iir_df1_mc_max_order(void) { return 8; }
void *llzs_stream_create(void) { return malloc(1); }
void llzs_stream_destroy(void *s) { free(s); }
void *llzs_event_create(void) { return malloc(1); }
void llzs_event_destroy(void *e) { free(e); }
'''


def gen_trace_stub():
    """STUB_HEAD, then every other function of llz_shim.h as a traced no-op: a kernel launch writes its name and arguments."""
    text = open(os.path.join(CSRC, "llz_shim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    done = set(re.findall(r"\b(llzs_\w+|llz_hip_\w+)\s*\(", STUB_HEAD))
    out = [STUB_HEAD]
    for m in re.finditer(r"\b(int|void|double|void \*)\s*\*?\s*(llzs_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        if name in done:
            continue
        done.add(name)
        fmt, vals = [name], []
        for arg in ([] if args == "void" else args.split(",")):
            ident = re.findall(r"[A-Za-z_]\w*", arg.split("[")[0])[-1]
            if ident == "stream":
                fmt.append("stream=%d"); vals.append("stream != NULL")
            elif "*" in arg or "[" in arg:
                fmt.append(ident + "=%s"); vals.append(f"dp({ident})")
            elif re.search(r"\b(float|double)\b", arg):
                fmt.append(ident + "=%.17g"); vals.append(f"(double){ident}")
            else:
                fmt.append(ident + "=%lld"); vals.append(f"(long long){ident}")
        body = "return 1;" if name.endswith("_fits") else ("return 0;" if ret != "void" else "")
        call = ", ".join(['"' + " ".join(fmt) + '"'] + vals)
        out.append(f"{ret} {name}({args}) {{ tr(1, {call}); {body} }}")
    return "\n".join(out) + "\n"


def build_driver(tmp_path, host_dir):
    stub = tmp_path / "trace_stub.c"
    stub.write_text(gen_trace_stub())
    exe = tmp_path / "host_calls"
    srcs = sorted(glob.glob(os.path.join(host_dir, "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "host_calls_driver.c"), str(stub)] + srcs + \
          ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("host_calls"), os.path.join(CSRC, "host"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)


def _scenarios(text):
    return {m.group(1): (int(m.group(2)), m.group(3), m.group(4)) for m in re.finditer(r"^scenario (\S+) lines (\d+) fnv (\w{16}) tables (\w{16})$", text, re.M)}


def test_every_scenario_makes_the_recorded_shim_calls(driver_run):
    r = driver_run
    assert "SCENARIOS_DONE" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = _scenarios(r.stdout)
    want = _scenarios(open(os.path.join(HERE, "host_calls_expected.txt")).read())
    assert len(want) == 152 and CHANGED_CALLS <= set(want)
    assert all(any(k.startswith(p) and k.endswith(".init") for k in want) for p in CHANGED_INITS)
    assert set(got) == set(want)
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, "\n".join(f"{k}: {got[k]} instead of {want[k]}" for k in differ)


def test_failed_allocations_are_refused_and_nothing_leaks(driver_run):
    r = driver_run
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "HOST_CALLS_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    # every init form once and every one-shot call: 53 scenarios; an allocation refused for each one they make: 207
    assert "fault injection: 207 refused allocations over 53 scenarios, 0 faults" in r.stdout
