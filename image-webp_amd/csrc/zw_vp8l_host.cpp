// zw_vp8l_host.cpp -- lossless (VP8L) files into the caller's device memory:
// the chunk pipeline between the host reader (zw_vp8l_dec.cpp, decode_coded) and
// the transform and store kernels (zw_vp8l_kernels.hip).
//
// A run of n files of one size is worked in chunks.  The host threads
// entropy-decode a chunk's files, one file per task, straight into one of two
// pinned staging sets laid out as the device sees the chunk (ll_layout): the
// ZwLlFrame table, for every (inverse step, transform type) the list of the
// frames whose step is of that type, then each frame's slot (coded image,
// transform data).  One copy uploads it; the inverse steps run in order, one
// launch per non-empty list; the store kernel writes the caller's tensor.  All
// of it is queued on the context's stream, so the device works chunk k while
// the host threads decode chunk k + 1 into the other staging set (a set is
// reused once its upload's event has completed).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/zwebp.h"
#include "zw_common.h"
#include "zw_host_internal.h"
#include "zw_vp8l_dec.h"

extern "C" {
hipError_t zwk_ll_inverse(hipStream_t s, const ZwLlChunk* C, uint32_t step, uint32_t type, const uint32_t* list,
                          int count);
hipError_t zwk_ll_store(hipStream_t s, const ZwLlChunk* C, int layout, int dtype, int channels, void* out,
                        const ZwY2rDev* P, int nframes);
}
bool zw_vp8l_hook_image(const zw_vp8l_image& im, uint32_t width, uint32_t height, zwvp8l::Coded& c);

namespace {

double ll_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// A chunk of cnt frames of w x h, in staging and on the device alike up to
// `upload`; the full-width buffers follow on the device only.
struct LlLayout {
    size_t lists;    // the 16 lists of cnt entries, after the table
    size_t slots;    // the first frame's slot
    size_t sstride;  // between slots: the pixels' room, then the data region
    size_t doff, dbytes;
    size_t upload;   // the bytes the upload copies
    size_t full, bstride, total;
};
LlLayout ll_layout(int cnt, size_t w, size_t h)
{
    LlLayout L;
    L.lists = (size_t)cnt * sizeof(ZwLlFrame);
    L.slots = al256(L.lists + (size_t)16 * cnt * sizeof(uint32_t));
    L.doff = al16(w * h * 4) + 16;
    // two sub-images of at most ceil(w / 4) x ceil(h / 4) pixels, a table of 256 entries, each 16-aligned
    L.dbytes = al16(2 * ((w + 3) / 4) * ((h + 3) / 4) * 4 + 1024 + 64);
    L.sstride = L.doff + L.dbytes;
    L.upload = L.slots + (size_t)cnt * L.sstride;
    L.full = al256(L.upload);
    L.bstride = al16(w * h * 4);
    L.total = L.full + (size_t)cnt * L.bstride;
    return L;
}

// Frame i's table entry and data region from its transforms (c passed inverse_sizes_ok).
void ll_describe(uint8_t* stage, const LlLayout& L, int i, const zwvp8l::Coded& c, bool has_alpha)
{
    ZwLlFrame& F = ((ZwLlFrame*)stage)[i];
    memset(&F, 0, sizeof F);
    F.tw = c.tw;
    F.has_alpha = has_alpha;
    F.nsteps = (uint32_t)c.tf.size();
    F.index_step = ZW_LL_NO_INDEX;
    uint8_t* data = stage + L.slots + (size_t)i * L.sstride + L.doff;
    size_t off = 0;
    uint32_t wk = c.width;  // the working width, in bitstream order
    for (uint32_t j = 0; j < F.nsteps; j++) {
        const zwvp8l::CodedTransform& t = c.tf[j];
        const uint32_t k = F.nsteps - 1 - j;  // the inverse order
        F.s[k].type = t.type;
        F.s[k].bits = t.bits;
        F.s[k].off = (uint32_t)off;
        // exactly what the kernels address (inverse_sizes_ok: the data holds it): at
        // most a sub-image of ceil(w / 4) x ceil(h / 4) pixels, or 1024 bytes
        size_t nb = 0;
        if (t.type == 3) {
            F.index_step = k;
            nb = (size_t)t.bits * 4;
            wk = zwvp8l::packed_width(wk, t.bits);
        } else if (t.type != 2) {
            nb = (size_t)((wk + (1u << t.bits) - 1) >> t.bits) * ((c.height + (1u << t.bits) - 1) >> t.bits) * 4;
        }
        if (nb) memcpy(data + off, t.data.data(), nb);
        off = al16(off + nb);
    }
}

// The lists of a staged chunk; nlist[step][type] = their lengths.
void ll_lists(uint8_t* stage, const LlLayout& L, int cnt, int nlist[4][4])
{
    memset(nlist, 0, sizeof(int) * 16);
    const ZwLlFrame* tab = (const ZwLlFrame*)stage;
    uint32_t* lists = (uint32_t*)(stage + L.lists);
    for (int i = 0; i < cnt; i++)
        for (uint32_t k = 0; k < tab[i].nsteps; k++) {
            const uint32_t type = tab[i].s[k].type;
            lists[(size_t)(k * 4 + type) * cnt + nlist[k][type]++] = (uint32_t)i;
        }
}

// Queues the chunk's upload and its inverse steps; *C = the chunk as the kernels take it.
int ll_enqueue(hipStream_t s, uint8_t* dev, const uint8_t* stage, const LlLayout& L, int cnt, size_t w, size_t h,
               const int nlist[4][4], hipEvent_t uploaded, hipEvent_t started, ZwLlChunk* C)
{
    HIPOK(hipMemcpyAsync(dev, stage, L.upload, hipMemcpyHostToDevice, s));
    if (uploaded) HIPOK(hipEventRecord(uploaded, s));
    if (started) HIPOK(hipEventRecord(started, s));  // (the transform kernels' time starts after the upload)
    C->slots = dev + L.slots;
    C->full = dev + L.full;
    C->tab = (const ZwLlFrame*)dev;
    C->sstride = L.sstride;
    C->doff = L.doff;
    C->bstride = L.bstride;
    C->w = (int)w;
    C->h = (int)h;
    const uint32_t* d_lists = (const uint32_t*)(dev + L.lists);
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t type = 0; type < 4; type++)
            HIPOK(zwk_ll_inverse(s, C, k, type, d_lists + (size_t)(k * 4 + type) * cnt, nlist[k][type]));
    return ZW_OK;
}

struct LlEvents {
    std::vector<hipEvent_t> ev;
    ~LlEvents()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int make(hipEvent_t* e)
    {
        HIPOK(hipEventCreate(e));
        ev.push_back(*e);
        return ZW_OK;
    }
};

}  // namespace

// n VP8L payloads of w x h into out (the run's first frame).  has_alpha[i]:
// channel 3 of frame i holds its decoded alpha (else 255).
int zw_ll_decode_run(zw_ctx* ctx, int n, const uint8_t* const* payload, const size_t* plen, const uint8_t* has_alpha,
                     uint32_t w, uint32_t h, const ZwLlOut& O)
{
    if (n <= 0 || w == 0 || h == 0 || w > 16384 || h > 16384) return ZW_EINVAL;
    HIPOK(hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    // the chunk: what about 320 MB of scratch (or the context's, if larger) hold, whole rounds of the host threads
    const LlLayout one = ll_layout(1, w, h);
    const size_t budget = std::max(ctx->set[0].scratch.cap, (size_t)320 << 20);
    int per = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / (one.sstride + one.bstride + 512)));
    const int nt = host_threads();
    if (per > nt) per -= per % nt;
    const LlLayout big = ll_layout(per, w, h);
    uint8_t* dev = (uint8_t*)ctx_scratch(ctx, big.total);
    uint8_t* stage[2] = {(uint8_t*)ctx->pin[PIN_VP8L0].reserve(big.upload),
                         n > per ? (uint8_t*)ctx->pin[PIN_VP8L1].reserve(big.upload) : nullptr};
    if (!dev || !stage[0] || (n > per && !stage[1])) return ZW_ENOMEM;
    LlEvents E;
    hipEvent_t uploaded[2] = {nullptr, nullptr};
    for (hipEvent_t& e : uploaded)
        if (int r = E.make(&e)) return r;
    struct Times {
        hipEvent_t e[3];  // upload done, transforms done, store done
    };
    std::vector<Times> times;
    double host_ms = 0;
    std::vector<int> rc;
    int result = ZW_OK;
    for (int first = 0, k = 0; first < n && result == ZW_OK; first += per, k++) {
        const int cnt = std::min(per, n - first), set = k & 1;
        const LlLayout L = ll_layout(cnt, w, h);
        if (k >= 2) HIPOK(hipEventSynchronize(uploaded[set]));  // the set's last upload has left it
        uint8_t* st = stage[set];
        rc.assign((size_t)cnt, ZW_OK);
        const double t0 = ll_now_ms();
        parallel_for(cnt, [&](int i) {
            try {
                zwvp8l::Coded c;
                uint8_t* px = st + L.slots + (size_t)i * L.sstride;
                rc[i] = zwvp8l::decode_coded(payload[first + i], plen[first + i], w, h, false, px, (size_t)w * h * 4, c);
                if (rc[i]) return;
                if (!zwvp8l::inverse_sizes_ok(c)) {
                    rc[i] = ZW_EBITSTREAM;
                    return;
                }
                ll_describe(st, L, i, c, has_alpha[first + i] != 0);
            } catch (const std::bad_alloc&) {
                rc[i] = ZW_ENOMEM;
            }
        });
        host_ms += ll_now_ms() - t0;
        for (int i = 0; i < cnt && result == ZW_OK; i++) result = rc[i];
        if (result) break;
        int nlist[4][4];
        ll_lists(st, L, cnt, nlist);
        Times T;
        for (hipEvent_t& e : T.e)
            if (int r = E.make(&e)) return r;
        ZwLlChunk C;
        if (int r = ll_enqueue(s, dev, st, L, cnt, w, h, nlist, uploaded[set], T.e[0], &C)) return r;
        HIPOK(hipEventRecord(T.e[1], s));
        HIPOK(zwk_ll_store(s, &C, O.layout, O.dtype, O.channels, O.data + (size_t)first * O.P.frame_stride * O.elsize,
                           &O.P, cnt));
        HIPOK(hipEventRecord(T.e[2], s));
        times.push_back(T);
    }
    HIPOK(hipStreamSynchronize(s));  // (also after an error: the chunks queued before it finish)
    ctx->ll_ms[0] += (float)host_ms;
    for (const Times& T : times) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, T.e[0], T.e[1]) == hipSuccess) ctx->ll_ms[1] += ms;
        if (hipEventElapsedTime(&ms, T.e[1], T.e[2]) == hipSuccess) ctx->ll_ms[2] += ms;
    }
    return result;
}

extern "C" int zw_decode_lossless_times(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    for (int i = 0; i < 3; i++) ms[i] = ctx->ll_ms[i];
    return ZW_OK;
}

extern "C" int zw_dbg_vp8l_inverse_device(zw_ctx* ctx, int n, const zw_vp8l_image* images, uint32_t width,
                                          uint32_t height, uint8_t* out)
{
    if (!ctx || n <= 0 || n > 4096 || !images || !out || width == 0 || height == 0 || width > 16384 || height > 16384)
        return ZW_EINVAL;
    const size_t w = width, h = height, fbytes = w * h * 4;
    try {
        std::vector<zwvp8l::Coded> cs((size_t)n);
        for (int i = 0; i < n; i++)
            if (!zw_vp8l_hook_image(images[i], width, height, cs[i])) return ZW_EINVAL;
        HIPOK(hipSetDevice(ctx->device));
        const LlLayout L = ll_layout(n, w, h);
        uint8_t* dev = (uint8_t*)ctx_scratch(ctx, L.total);
        uint8_t* st = (uint8_t*)ctx->pin[PIN_VP8L0].reserve(L.upload);
        if (!dev || !st) return ZW_ENOMEM;
        for (int i = 0; i < n; i++) {
            memcpy(st + L.slots + (size_t)i * L.sstride, images[i].coded, (size_t)cs[i].tw * h * 4);
            ll_describe(st, L, i, cs[i], true);
        }
        int nlist[4][4];
        ll_lists(st, L, n, nlist);
        hipStream_t s = ctx_stream(ctx);
        ZwLlChunk C;
        if (int r = ll_enqueue(s, dev, st, L, n, w, h, nlist, nullptr, nullptr, &C)) return r;
        HIPOK(hipStreamSynchronize(s));
        for (int i = 0; i < n; i++) {
            const ZwLlFrame& F = ((const ZwLlFrame*)st)[i];
            const uint8_t* src = F.index_step != ZW_LL_NO_INDEX ? C.full + (size_t)i * C.bstride
                                                                : C.slots + (size_t)i * C.sstride;
            HIPOK(hipMemcpy(out + (size_t)i * fbytes, src, fbytes, hipMemcpyDeviceToHost));
        }
    } catch (const std::bad_alloc&) {
        return ZW_ENOMEM;
    }
    return ZW_OK;
}
