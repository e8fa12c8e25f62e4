/*
 * fir_tables.c -- the tap tables of the separable FIR kernels (kernels/fir_ops.hip and the sweeps): planned on the host,
 * kept on the device, reused.
 *
 * One tap table per axis: a table depends only on (kind, factor or taps, target range, source range), which repeat from
 * frame to frame, so in steady state a blur, a resample or a scaler pass is one kernel launch with no host-side planning,
 * no upload, no sync.  The dispatchers (scale.c) ask for a table by what it computes (internal.h cvs_fir_table_*); the key
 * it is cached under is built here only.
 */
#define _GNU_SOURCE
#include "internal.h"
#include <limits.h>
#include <math.h>
#include <pthread.h>

typedef struct {
    int t0, t1;            /* target lines covered by the table */
    int stride;
    int *ntaps, *tap_src;
    float *taps;
    int used_lo, used_hi;  /* target lines that received at least one tap */
} tap_table;

static void table_free(tap_table *tb) { free(tb->ntaps); free(tb->tap_src); free(tb->taps); memset(tb, 0, sizeof *tb); }

static int table_alloc(tap_table *tb, int t0, int t1, int stride) {
    memset(tb, 0, sizeof *tb);
    tb->t0 = t0; tb->t1 = t1; tb->stride = stride > 0 ? stride : 1;
    tb->used_lo = INT_MAX; tb->used_hi = INT_MIN;
    size_t lines = t1 >= t0 ? (size_t)(t1 - t0 + 1) : 0;
    tb->ntaps = calloc(lines ? lines : 1, sizeof(int));
    tb->tap_src = calloc((lines ? lines : 1) * (size_t)tb->stride, sizeof(int));
    tb->taps = calloc((lines ? lines : 1) * (size_t)tb->stride, sizeof(float));
    if (!tb->ntaps || !tb->tap_src || !tb->taps) { table_free(tb); return -1; }
    return 0;
}

static inline void table_add(tap_table *tb, int t, int s, float c) {
    int row = t - tb->t0, k = tb->ntaps[row];
    if (k < tb->stride) { tb->tap_src[(size_t)row * tb->stride + k] = s; tb->taps[(size_t)row * tb->stride + k] = c; }
    tb->ntaps[row] = k + 1;
}

/* widest triangle the per-line generator can return (video_scale.c:52-57) */
static int triangle_cap(float factor) {
    float dummy = factor;
    fir_filter probe = { &dummy, 0, 0 };
    filter_createTriangle(factor, 0.0f, &probe);
    return probe.width + 3;
}

/* Tap table of one triangle pass.  count_touch: whether an in-range tap marks its target line as
 * used even when the other axis is empty (true for the vertical pass, :88-89; the horizontal pass
 * only marks inside its row loop, :186-187). */
static int plan_triangle(tap_table *tb, float tmin, float smin, float factor, int s0, int s1, int t0, int t1, bool count_touch, int contracted) {
    const int cap = triangle_cap(factor);
    float *buf = malloc(sizeof(float) * (size_t)cap);
    if (!buf) return -1;
    fir_filter f = { buf, 0, 0 };
    int rc = 0;
    if (factor > 1.0f) {
        /* scatter form: how many source lines can land on one target line?  count first */
        int lines = t1 >= t0 ? t1 - t0 + 1 : 0;
        int *count = calloc((size_t)(lines ? lines : 1), sizeof(int));
        if (!count) { free(buf); return -1; }
        for (int pass = 0; pass < 2 && rc == 0; pass++) {
            if (pass == 1) {
                int most = 1;
                for (int i = 0; i < lines; i++) if (count[i] > most) most = count[i];
                rc = table_alloc(tb, t0, t1, most);
                if (rc != 0) break;
            }
            for (int s = s0; s <= s1; s++) {
                float centre_f = madd_as(contracted, s - smin, factor, tmin);       /* video_scale.c:65 */
                int centre = (int)floor(centre_f);
                f.width = cap;
                filter_createTriangle(factor, centre_f - centre, &f);
                for (int k = 0; k < f.width; k++) {
                    int t = centre - f.center + k;
                    if (t < t0 || t > t1) continue;
                    if (pass == 0) count[t - t0]++;
                    else {
                        table_add(tb, t, s, buf[k]);
                        if (count_touch) { if (t < tb->used_lo) tb->used_lo = t; if (t > tb->used_hi) tb->used_hi = t; }
                    }
                }
            }
        }
        free(count);
    } else {
        rc = table_alloc(tb, t0, t1, cap);
        for (int t = t0; rc == 0 && t <= t1; t++) {
            float centre_f = (t - tmin) / factor + smin;
            int centre = (int)floor(centre_f);
            f.width = cap;
            filter_createTriangle(factor, centre_f - centre, &f);
            for (int k = 0; k < f.width; k++) {
                int s = centre - f.center + k;
                if (s < s0 || s > s1) continue;
                table_add(tb, t, s, buf[k]);
                if (count_touch) { if (t < tb->used_lo) tb->used_lo = t; if (t > tb->used_hi) tb->used_hi = t; }
            }
        }
    }
    free(buf);
    return rc;
}

/* ---------------------------------------------------------------- FIR blur (repo-defined, DESIGN.md "A11")
 * Odd or even tap count, centre = ntaps/2; horizontal then vertical; accumulate from 0.0f in
 * ascending tap order; taps falling outside the source's current_window are skipped; output window =
 * source.current ∩ target.full. */
static int plan_blur(tap_table *tb, int t0, int t1, int s0, int s1, const float *taps, int ntaps) {
    int rc = table_alloc(tb, t0, t1, ntaps);
    const int c = ntaps / 2;
    for (int t = t0; rc == 0 && t <= t1; t++)
        for (int k = 0; k < ntaps; k++) {
            int sidx = t - c + k;
            if (sidx < s0 || sidx > s1) continue;
            table_add(tb, t, sidx, taps[k]);
        }
    tb->used_lo = t0; tb->used_hi = t1;
    return rc;
}

/* ---------------------------------------------------------------- Lanczos gather resample (repo-defined)
 * Per target line the taps come from filter_createLanczos(factor, kernel_size, frac(centre)) with
 * centre = t / factor (origin 0 on both sides); x pass then y pass; f32 accumulate from 0. */
static int plan_lanczos(tap_table *tb, int t0, int t1, int s0, int s1, float factor, int ksize) {
    fir_filter probe = { NULL, 0, 0 };
    filter_createLanczos(factor, ksize, 0.0f, &probe);
    int cap = probe.width + 3;
    filter_free(&probe);
    int rc = table_alloc(tb, t0, t1, cap);
    for (int t = t0; rc == 0 && t <= t1; t++) {
        float centre_f = (float)t / factor;
        int centre = (int)floor(centre_f);
        fir_filter f = { NULL, 0, 0 };
        filter_createLanczos(factor, ksize, centre_f - centre, &f);
        if (!f.coeff) { rc = -1; break; }
        for (int k = 0; k < f.width; k++) {
            int sidx = centre - f.center + k;
            if (sidx < s0 || sidx > s1) continue;
            table_add(tb, t, sidx, f.coeff[k]);
        }
        filter_free(&f);
    }
    tb->used_lo = t0; tb->used_hi = t1;
    return rc;
}

/* ---------------------------------------------------------------- the device cache */

enum { KIND_BLUR = 1, KIND_LANCZOS = 2, KIND_TRIANGLE = 3 };

typedef struct {
    int kind;                 /* KIND_* */
    uint32_t fbits;           /* lanczos, triangle: factor bits */
    int ksize;                /* lanczos: kernel size; blur: tap count; triangle: count_touch */
    uint64_t taps_hash;       /* blur: FNV-1a of the tap values; triangle: tmin bits << 32 | smin bits */
    int t0, t1, s0, s1;
    int tile;                 /* tile edge along this axis */
    int flavour;              /* triangle, enlarging: the arithmetic flavour the line centres were computed in (0 elsewhere) */
} axis_key;

typedef struct {
    axis_key key;
    int valid;
    int pins;                 /* calls that hold the table's address and have not enqueued their launch yet (+ captured graphs) */
    uint64_t stamp;
    char *dev;                /* one block: ntaps | src | taps | foot */
    cvk_fir_axis axis;
    int max_foot;
    int used_lo, used_hi;     /* target lines that receive at least one tap (the window the pass reports) */
} axis_entry;

typedef struct { const float *taps; float factor, tmin, smin; int contracted; } axis_plan;    /* what the planner of the key's kind needs */

/* The tables live on the device: one cache per device context (runtime.c), one lock over all of them. */
#define AXIS_CACHE 128
#define AXIS_RETIRED 64
typedef struct { axis_entry e[AXIS_CACHE]; uint64_t clock; char *retired[AXIS_RETIRED]; int nretired; } axis_cache;
static axis_cache g_axis_of[CVS_MAX_CONTEXTS];
#define g_axis (g_axis_of[cvs_ctx()].e)
#define g_axis_clock (g_axis_of[cvs_ctx()].clock)
#define g_retired (g_axis_of[cvs_ctx()].retired)
#define g_nretired (g_axis_of[cvs_ctx()].nretired)
static pthread_mutex_t g_axis_lock = PTHREAD_MUTEX_INITIALIZER;

/* keys are compared with memcmp: build them from zeroed storage so that padding is defined */
static axis_key make_key(int kind, uint32_t fbits, int ksize, uint64_t taps_hash, int t0, int t1, int s0, int s1, int tile) {
    axis_key k;
    memset(&k, 0, sizeof k);
    k.kind = kind; k.fbits = fbits; k.ksize = ksize; k.taps_hash = taps_hash;
    k.t0 = t0; k.t1 = t1; k.s0 = s0; k.s1 = s1; k.tile = tile;
    return k;
}

static uint64_t fnv1a(const void *p, size_t n) {
    const unsigned char *b = p;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

/* the source lines target lines i0 .. i1 - 1 of the table read, from the lowest first tap to the highest last one:
 * *first .. *last (0 .. -1 when none has a tap); returns how many */
static int table_reach(const tap_table *tb, const int *ntaps, int i0, int i1, int *first, int *last) {
    int lo = INT_MAX, hi = INT_MIN;
    for (int i = i0; i < i1; i++) {
        if (!ntaps[i]) continue;
        const int *src = tb->tap_src + (size_t)i * tb->stride;
        if (src[0] < lo) lo = src[0];
        if (src[ntaps[i] - 1] > hi) hi = src[ntaps[i] - 1];
    }
    if (hi < lo) { lo = 0; hi = -1; }
    *first = lo; *last = hi;
    return hi - lo + 1;
}

/* device copy of one axis table (+ per-tile footprints); returns 0 and fills *out on success */
static int axis_upload(const tap_table *tb, int tile, axis_entry *e) {
    const int lines = tb->t1 >= tb->t0 ? tb->t1 - tb->t0 + 1 : 0;
    const int tiles = (lines + tile - 1) / tile;
    const int tiles_pad = ((tiles ? tiles : 1) + 3) & ~3;          /* kernels read four entries at once: spare ones touch nothing */
    int *foot = malloc(sizeof(int) * 2 * (size_t)tiles_pad);
    int *ntaps = malloc(sizeof(int) * (size_t)(lines ? lines : 1));
    if (!foot || !ntaps) { free(foot); free(ntaps); return -1; }
    int max_foot = 0;
    for (int i = 0; i < lines; i++) ntaps[i] = tb->ntaps[i] < tb->stride ? tb->ntaps[i] : tb->stride;
    for (int t = 0; t < tiles; t++) {
        const int w = table_reach(tb, ntaps, t * tile, (t + 1) * tile < lines ? (t + 1) * tile : lines, &foot[2 * t], &foot[2 * t + 1]);
        if (w > max_foot) max_foot = w;
    }
    for (int t = tiles; t < tiles_pad; t++) { foot[2 * t] = 0; foot[2 * t + 1] = -1; }
    /* what the streaming kernel needs to know about the table */
    int max_taps = 0, wide_foot = 0, max_active = 0, streamable = 1;
    {
        int prev_a = INT_MIN, prev_b = INT_MIN;
        for (int i = 0; i < lines; i++) {
            const int n = ntaps[i];
            if (n > max_taps) max_taps = n;
            if (!n) continue;
            const int *src = tb->tap_src + (size_t)i * tb->stride;
            for (int k = 1; k < n; k++) if (src[k] != src[0] + k) streamable = 0;
            if (src[0] < prev_a || src[n - 1] < prev_b) streamable = 0;
            prev_a = src[0]; prev_b = src[n - 1];
        }
        for (int g = 0; g < lines; g += 128) {              /* strips of 128 lines (tile_vh_ops.hip's target columns) */
            int first, last;
            const int w = table_reach(tb, ntaps, g, g + 128 < lines ? g + 128 : lines, &first, &last);
            if (w > wide_foot) wide_foot = w;
        }
        if (streamable) {
            int j = 0;
            for (int i = 0; i < lines; i++) {
                if (!ntaps[i]) continue;
                const int b = tb->tap_src[(size_t)i * tb->stride + ntaps[i] - 1];
                if (j < i) j = i;
                while (j + 1 < lines) {                       /* furthest later line that starts at or before b */
                    int nxt = j + 1;
                    while (nxt < lines && !ntaps[nxt]) nxt++;
                    if (nxt >= lines || tb->tap_src[(size_t)nxt * tb->stride] > b) break;
                    j = nxt;
                }
                if (j - i + 1 > max_active) max_active = j - i + 1;
            }
        }
    }
    /* source lines under any CVK_FIR_TVH_LINES consecutive target lines (tile_vh_ops.hip sizes its LDS rows by it); in a
     * streamable table the lowest first tap is the first line's and the highest last tap the last line's */
    int span_lines[3] = { 0, 0, 0 };
    for (int g = 0; streamable && g < 3; g++) {
        const int run = CVK_FIR_TVH_LINES << g;
        for (int i = 0; i < lines; i++) {
            int first, last;
            const int w = table_reach(tb, ntaps, i, i + run < lines ? i + run : lines, &first, &last);
            if (w > span_lines[g]) span_lines[g] = w;
        }
    }
    /* the table by TARGET line in one record each (kernels.h cvk_fir_axis.lrec): one scalar load per line */
    uint32_t *lrec = NULL;
    if (streamable && max_taps >= 1 && max_taps <= CVK_FIR_LREC - 2) {
        lrec = calloc(((size_t)lines + 1) * CVK_FIR_LREC, sizeof *lrec);      /* + one spare record: the kernel loads a line ahead */
        if (!lrec) { free(foot); free(ntaps); return -1; }
        for (int i = 0; i <= lines; i++) {
            uint32_t *r = lrec + (size_t)i * CVK_FIR_LREC;
            const int n = i < lines ? ntaps[i] : 0;
            r[0] = (uint32_t)n;
            r[1] = n ? (uint32_t)tb->tap_src[(size_t)i * tb->stride] : (uint32_t)INT_MIN;     /* no taps: never moves the window */
            for (int k = 0; k < n; k++) memcpy(&r[2 + k], &tb->taps[(size_t)i * tb->stride + k], 4);
        }
    }
    /* ... and, for short lists, by target line in one aligned read each (kernels.h cvk_fir_axis.pack) */
    const int pack_width = max_taps >= 1 && max_taps <= 2 ? 2 : max_taps <= 4 && max_taps >= 1 ? 4 : 0;
    uint32_t *pack = NULL;
    if (pack_width) {
        pack = malloc((size_t)(lines ? lines : 1) * 2 * (size_t)pack_width * sizeof *pack);
        if (!pack) { free(foot); free(ntaps); free(lrec); return -1; }
        for (int i = 0; i < lines; i++) {
            uint32_t *r = pack + (size_t)i * 2 * pack_width;
            for (int k = 0; k < pack_width; k++) {
                const bool has = k < ntaps[i];
                const float zero = 0.0f;
                r[k] = has ? (uint32_t)tb->tap_src[(size_t)i * tb->stride + k] : (uint32_t)INT_MIN;
                memcpy(&r[pack_width + k], has ? &tb->taps[(size_t)i * tb->stride + k] : &zero, 4);
            }
        }
    }
    const size_t n_l = (size_t)(lines ? lines : 1), n_t = n_l * (size_t)tb->stride;
    const size_t off_src = CVK_AXIS_OFF_SRC(lines), off_tap = CVK_AXIS_OFF_TAPS(lines, tb->stride), off_foot = CVK_AXIS_OFF_FOOT(lines, tb->stride);
    const size_t off_lrec = off_foot + ((sizeof(int) * 2 * (size_t)tiles_pad + 255) & ~(size_t)255);
    const size_t lrec_bytes = lrec ? ((size_t)lines + 1) * CVK_FIR_LREC * sizeof *lrec : 0;
    const size_t off_pack = off_lrec + (((lrec_bytes ? lrec_bytes : 4) + 255) & ~(size_t)255);
    const size_t pack_bytes = pack ? n_l * 2 * (size_t)pack_width * sizeof *pack : 0;
    const size_t total = off_pack + (pack_bytes ? pack_bytes : 4);
    char *dev = NULL;
    hipError_t err = hipMalloc((void **)&dev, total);
    if (err == hipSuccess) err = hipMemcpy(dev, ntaps, n_l * sizeof(int), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev + off_src, tb->tap_src, n_t * sizeof(int), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev + off_tap, tb->taps, n_t * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dev + off_foot, foot, sizeof(int) * 2 * (size_t)tiles_pad, hipMemcpyHostToDevice);
    if (err == hipSuccess && lrec_bytes) err = hipMemcpy(dev + off_lrec, lrec, lrec_bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess && pack_bytes) err = hipMemcpy(dev + off_pack, pack, pack_bytes, hipMemcpyHostToDevice);
    free(foot); free(ntaps); free(lrec); free(pack);
    if (err != hipSuccess) { if (dev) hipFree(dev); cvs_set_error("FIR table upload: %s", hipGetErrorString(err)); return -1; }
    e->dev = dev;
    e->axis.ntaps = (const int *)dev;
    e->axis.src = (const int *)(dev + off_src);
    e->axis.taps = (const float *)(dev + off_tap);
    e->axis.foot = (const int *)(dev + off_foot);
    e->axis.stride = tb->stride; e->axis.lines = lines;
    e->axis.max_taps = max_taps; e->axis.wide_foot = wide_foot; e->axis.max_active = max_active; e->axis.streamable = streamable;
    e->axis.lrec = lrec_bytes ? (const uint32_t *)(dev + off_lrec) : NULL;
    e->axis.pack = pack_bytes ? (const uint32_t *)(dev + off_pack) : NULL; e->axis.pack_width = pack_bytes ? pack_width : 0;
    memcpy(e->axis.span_lines, span_lines, sizeof span_lines);
    e->max_foot = max_foot;
    return 0;
}

/* Device blocks of evicted (or lost-the-race) tables.  A kernel on ANY stream may still be reading an evicted table, so
 * its block is parked here instead of freed; when the list is full ONE device-wide wait -- outside every lock -- makes all
 * of them free at once.  (The first version waited for the whole device under the cache lock on every eviction: an
 * animated zoom, which misses on every frame, stalled all streams and all pull-queue workers once per frame.) */

static void retire_block(char *dev) {           /* g_axis_lock NOT held */
    if (!dev) return;
    char *drain[AXIS_RETIRED];
    int n = 0;
    pthread_mutex_lock(&g_axis_lock);
    if (g_nretired == AXIS_RETIRED) { memcpy(drain, g_retired, sizeof drain); n = g_nretired; g_nretired = 0; }
    g_retired[g_nretired++] = dev;
    pthread_mutex_unlock(&g_axis_lock);
    if (n) {
        (void)hipDeviceSynchronize();           /* every launch enqueued before this point has finished */
        for (int i = 0; i < n; i++) (void)hipFree(drain[i]);
    }
}

/* hands out slot `slot` of this context's cache (g_axis_lock held), pinned */
static void take_entry(int slot, cvs_fir_table *out) {
    axis_entry *e = &g_axis[slot];
    e->stamp = ++g_axis_clock;
    e->pins++;
    out->axis = e->axis; out->max_foot = e->max_foot;
    out->used_lo = e->used_lo; out->used_hi = e->used_hi;
    out->pin = cvs_ctx() * AXIS_CACHE + slot;
}

/* cached table for one axis.  The entry comes back PINNED (out->pin): it cannot be evicted until cvs_fir_table_release()
 * says the launch that reads it is on its stream.  The lock covers table look-ups and slot bookkeeping only: planning, the
 * allocation and the upload of a missing table run outside it, and nothing under it calls back into the error log. */
static int axis_get(const axis_key *key, const axis_plan *pl, cvs_fir_table *out) {
    out->pin = -1;
    pthread_mutex_lock(&g_axis_lock);
    for (int i = 0; i < AXIS_CACHE; i++) {
        if (g_axis[i].valid && memcmp(&g_axis[i].key, key, sizeof *key) == 0) {
            take_entry(i, out);
            pthread_mutex_unlock(&g_axis_lock);
            return 0;
        }
    }
    pthread_mutex_unlock(&g_axis_lock);

    /* miss: build the table without holding anything */
    tap_table tb;
    int rc = key->kind == KIND_BLUR ? plan_blur(&tb, key->t0, key->t1, key->s0, key->s1, pl->taps, key->ksize)
           : key->kind == KIND_LANCZOS ? plan_lanczos(&tb, key->t0, key->t1, key->s0, key->s1, pl->factor, key->ksize)
           : plan_triangle(&tb, pl->tmin, pl->smin, pl->factor, key->s0, key->s1, key->t0, key->t1, key->ksize != 0, pl->contracted);
    if (rc != 0) { cvs_set_error("FIR planning: out of memory"); return -1; }
    axis_entry fresh;
    memset(&fresh, 0, sizeof fresh);
    fresh.used_lo = tb.used_lo; fresh.used_hi = tb.used_hi;
    rc = axis_upload(&tb, key->tile, &fresh);
    table_free(&tb);
    if (rc != 0) return -1;                                 /* axis_upload has logged why */
    fresh.key = *key; fresh.valid = 1;

    char *lost = NULL, *evicted = NULL;
    pthread_mutex_lock(&g_axis_lock);
    int slot = -1, victim = -1;
    for (int i = 0; i < AXIS_CACHE; i++) {
        if (g_axis[i].valid && memcmp(&g_axis[i].key, key, sizeof *key) == 0) { slot = i; break; }     /* another thread was faster */
        if (g_axis[i].valid && g_axis[i].pins > 0) continue;
        if (victim < 0 || (g_axis[victim].valid && (!g_axis[i].valid || g_axis[i].stamp < g_axis[victim].stamp))) victim = i;
    }
    if (slot >= 0) {
        lost = fresh.dev;                                   /* never read by any kernel, still parked like the others */
        take_entry(slot, out);
    } else if (victim >= 0) {
        if (g_axis[victim].valid) evicted = g_axis[victim].dev;
        g_axis[victim] = fresh;
        take_entry(victim, out);
    }
    pthread_mutex_unlock(&g_axis_lock);
    retire_block(lost);
    retire_block(evicted);
    if (slot < 0 && victim < 0) {
        retire_block(fresh.dev);
        cvs_set_error("FIR tables: every cache slot is held by a launch in preparation or a captured graph");
        return -1;
    }
    return 0;
}

/* `slot`: context * AXIS_CACHE + entry (a graph may be destroyed by a thread bound to another context) */
static void axis_unpin(void *slot) {
    const int id = (int)(intptr_t)slot;
    pthread_mutex_lock(&g_axis_lock);
    g_axis_of[id / AXIS_CACHE].e[id % AXIS_CACHE].pins--;
    pthread_mutex_unlock(&g_axis_lock);
}

/* the launch that reads the table is enqueued on `s` (or failed): let go of it, or hand the hold to the graph being captured */
void cvs_fir_table_release(cvs_fir_table *t, hipStream_t s) {
    if (t->pin < 0) return;
    if (!cvs_capture_hold(s, axis_unpin, (void *)(intptr_t)t->pin)) axis_unpin((void *)(intptr_t)t->pin);
    t->pin = -1;
}

int cvs_fir_table_blur(const float *taps, int ntaps, int t0, int t1, int s0, int s1, int tile, cvs_fir_table *out) {
    const axis_key key = make_key(KIND_BLUR, 0, ntaps, fnv1a(taps, sizeof(float) * (size_t)ntaps), t0, t1, s0, s1, tile);
    const axis_plan pl = { taps, 0.0f, 0.0f, 0.0f, 0 };
    return axis_get(&key, &pl, out);
}

int cvs_fir_table_lanczos(float factor, int ksize, int t0, int t1, int s0, int s1, int tile, cvs_fir_table *out) {
    uint32_t fb;
    memcpy(&fb, &factor, 4);
    const axis_key key = make_key(KIND_LANCZOS, fb, ksize, 0, t0, t1, s0, s1, tile);
    const axis_plan pl = { NULL, factor, 0.0f, 0.0f, 0 };
    return axis_get(&key, &pl, out);
}

int cvs_fir_table_triangle(float tmin, float smin, float factor, int s0, int s1, int t0, int t1, bool count_touch, cvs_fir_table *out) {
    uint32_t fb, tb, sb;
    memcpy(&fb, &factor, 4); memcpy(&tb, &tmin, 4); memcpy(&sb, &smin, 4);
    axis_key key = make_key(KIND_TRIANGLE, fb, count_touch ? 1 : 0, ((uint64_t)tb << 32) | sb, t0, t1, s0, s1, CVK_FIR2D_TILE_X);
    /* only the enlarging form has a product and a sum in one expression (the reducing form divides, video_scale.c:95) */
    const int contracted = factor > 1.0f && cvs_arith() == CVS_ARITH_CONTRACTED;
    key.flavour = contracted;
    const axis_plan pl = { NULL, factor, tmin, smin, contracted };
    return axis_get(&key, &pl, out);
}
