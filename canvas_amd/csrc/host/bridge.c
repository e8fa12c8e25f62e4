/*
 * bridge.c -- host frames and coded planes through HBM around a `_dev` entry (internal.h "bridge.c").
 *
 * Every reference-named entry point on host memory is the same sequence: enter, pick the thread's stream, give each buffer
 * a pooled device block (uploaded only where the caller says it has pixels; one block where two arguments are the same host
 * buffer), call the `_dev` twin, download the output, wait, free.  That sequence lives here once; frames.c, scale.c,
 * color.c, dv.c and mpeg2.c say which buffers and which twin.
 */
#include "internal.h"

int cvs_bridge_open(cvs_bridge *b) {
    memset(b, 0, sizeof *b);
    b->rc = cvs_enter();
    if (b->rc == 0) b->stream = cvs_pick_stream(NULL);
    return b->rc;
}

static int bridge_upload(cvs_bridge *b, int i) {
    const cvs_staged *st = &b->blk[i].st;
    b->blk[i].uploaded = 1;
    if (st->dev) CVS_HIP(hipMemcpyAsync(st->dev, b->blk[i].host, st->bytes, hipMemcpyHostToDevice, b->stream));
    return 0;
}

void *cvs_bridge_frame(cvs_bridge *b, const void *host, size_t bytes, int flags) {
    if (b->rc != 0) return NULL;
    int i = (flags & CVS_BRIDGE_PRIVATE) ? b->n : 0;
    while (i < b->n && (b->blk[i].host != host || b->blk[i].st.bytes != bytes)) i++;
    if (i == b->n) {
        if (b->n == CVS_BRIDGE_BLOCKS) { cvs_set_error("host bridge: more than %d buffers in one call", CVS_BRIDGE_BLOCKS); b->rc = -1; return NULL; }
        b->blk[i].host = host;
        b->rc = cvs_stage_in(&b->blk[i].st, host, bytes, 0, b->stream);
        b->n++;                                           /* counted even when it failed: close frees what there is */
    }
    if (b->rc == 0 && (flags & CVS_BRIDGE_UPLOAD) && !b->blk[i].uploaded) b->rc = bridge_upload(b, i);
    return b->blk[i].st.dev;
}

void cvs_bridge_planes(cvs_bridge *b, coded_image *dev, const coded_image *host, const int lines[3], bool upload) {
    size_t bytes[3], off[3], total = 0;
    for (int p = 0; p < 3; p++) {
        bytes[p] = (size_t)max(host->stride[p], 0) * (size_t)max(lines[p], 0);
        off[p] = total;
        total += (bytes[p] + 255) & ~(size_t)255;
    }
    char *block = cvs_bridge_frame(b, NULL, total ? total : 1, CVS_BRIDGE_PRIVATE);
    *dev = *host;
    for (int p = 0; p < 3; p++) {
        dev->data[p] = block ? block + off[p] : NULL;
        dev->line_count[p] = lines[p];
        if (upload && b->rc == 0) b->rc = cvs_memcpy_h2d(dev->data[p], host->data[p], bytes[p], b->stream);
    }
}

void cvs_bridge_planes_back(cvs_bridge *b, coded_image *host, const coded_image *dev) {
    for (int p = 0; p < 3 && b->rc == 0; p++)
        b->rc = cvs_memcpy_d2h(host->data[p], dev->data[p], (size_t)dev->stride[p] * (size_t)dev->line_count[p], b->stream);
}

static cvs_staged *bridge_find(cvs_bridge *b, const void *host) {
    for (int i = 0; i < b->n; i++)
        if (b->blk[i].host == host) return &b->blk[i].st;
    cvs_set_error("host bridge: the output buffer was never added");
    b->rc = -1;
    return NULL;
}

int cvs_bridge_pull_window(cvs_bridge *b, void *host, const box2i *full, const box2i *window, size_t px) {
    const cvs_staged *st = b->rc == 0 ? bridge_find(b, host) : NULL;
    if (!st) return b->rc;
    const size_t pitch = (size_t)cvs_box_width(full) * px;
    const size_t at = (size_t)(window->min.y - full->min.y) * pitch + (size_t)(window->min.x - full->min.x) * px;
    if (hipMemcpy2DAsync((char *)host + at, pitch, (const char *)st->dev + at, pitch, (size_t)cvs_box_width(window) * px,
                         (size_t)cvs_box_height(window), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
        hipStreamSynchronize(b->stream) != hipSuccess)
        b->rc = -1;
    return b->rc;
}

int cvs_bridge_close(cvs_bridge *b, void *out_host) {
    cvs_staged *out = b->rc == 0 && out_host ? bridge_find(b, out_host) : NULL;
    if (out) b->rc = cvs_stage_out(out, out_host, b->stream);
    for (int i = 0; i < b->n; i++) cvs_stage_free(&b->blk[i].st);
    b->n = 0;
    return b->rc;
}

int cvs_planes_check(const coded_image *image, int w, int h, int cw, int ch) {
    if (!image || !image->data[0] || !image->data[1] || !image->data[2]) return CVS_PLANES_MISSING;
    return image->stride[0] >= w && image->stride[1] >= cw && image->stride[2] >= cw && image->line_count[0] >= h && image->line_count[1] >= ch &&
           image->line_count[2] >= ch ? CVS_PLANES_OK : CVS_PLANES_SMALL;
}
