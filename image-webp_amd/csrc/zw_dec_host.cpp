// zw_dec_host.cpp -- VP8 keyframe decoder, device side: the chunk pipeline that
// feeds the host parser's packed MB records (zw_dec_parse.cpp) or the device
// token parse's (zw_dec_tokens.hip) to the reconstruction / loop filter kernels
// and brings the planes or packed RGB(A) back, or converts them straight into
// the caller's device memory (zw_vp8_decode_batch_device), with the alpha planes
// of lossy files that carry an ALPH chunk on request (zw_webp_decode_batch_device:
// host zw_vp8l_dec.cpp, device zw_alpha_kernels.hip).
//
//   host  : zw_dec_parse.cpp (headers, modes, tokens -> one packed record per
//           macroblock; no device code there).
//   device: k_dec_recon (dequant, iWHT, iDCT, prediction) and k_loopfilter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <new>
#include <string>
#include <vector>

#include "../../include/zwebp.h"
#include "zw_common.h"
#include "zw_dec_parse.h"
#include "zw_host_internal.h"
#include "zw_progress.h"
#include "zw_vp8l_dec.h"

extern "C" {
hipError_t zwk_dec_recon(hipStream_t s, const uint8_t* recs, const uint32_t* moff, const uint64_t* fbase,
                         const void* quant, uint8_t* Y, uint8_t* U, uint8_t* V, uint8_t* flags, int mbw, int mbh,
                         size_t ysz, size_t csz, int nframes, uint8_t* tiles);
hipError_t zwk_yuv2rgb(hipStream_t s, const uint8_t* Y, const uint8_t* U, const uint8_t* V, size_t ysz, size_t csz,
                       int w, int h, int ys, int cs, int bpp, int fancy, uint8_t* out, int nframes);
hipError_t zwk_yuv2rgb_dev(hipStream_t s, const uint8_t* Y, const uint8_t* U, const uint8_t* V, size_t ysz, size_t csz,
                           int w, int h, int ys, int cs, int layout, int dtype, int channels, int fancy, void* out,
                           const ZwY2rDev* P, int nframes);
hipError_t zwk_yuv2rgb_resize(hipStream_t s, const uint8_t* Y, const uint8_t* U, const uint8_t* V, size_t ysz,
                              size_t csz, int w, int h, int ys, int cs, int layout, int dtype, int channels, int fancy,
                              void* out, const ZwY2rDev* P, const ZwResizeFrame* tab, int ow, int oh, int nframes);
hipError_t zwk_yuv2rgb_resize_aa(hipStream_t s, const uint8_t* Y, const uint8_t* U, const uint8_t* V, size_t ysz,
                                 size_t csz, int w, int h, int ys, int cs, int layout, int dtype, int channels, int fancy,
                                 void* out, const ZwY2rDev* P, const ZwResizeFrame* tab, uint32_t* tables,
                                 const ZwAaTables* L, int ow, int oh, int nframes);
hipError_t zwk_dec_rows(hipStream_t s, int phase, const uint8_t* recs, const uint32_t* moff, const uint64_t* fbase,
                        const void* quant, uint8_t* Y, uint8_t* U, uint8_t* V, uint8_t* flags, const ZwFilterParams* fp,
                        int mbw, int mbh, size_t ysz, size_t csz, int nframes, int* rowsync, uint8_t* borders, int rows);
hipError_t zwk_dec_rows_init(hipStream_t s, int* rowsync, int mbh, int nframes);
size_t zw_dec_rows_sync_bytes(int mbh, int nframes);
size_t zw_dec_rows_border_bytes(int mbw, int nframes);
hipError_t zwk_loopfilter(hipStream_t s, uint8_t* Y, uint8_t* U, uint8_t* V, const uint8_t* flags,
                          const ZwFilterParams* fp, size_t ysz, size_t csz, int nframes, int mbw, const uint8_t* tiles);
hipError_t zwk_dec_tok_count(hipStream_t s, const uint8_t* blob, const ZwTokFrame* tf, const uint8_t* probs,
                             const uint8_t* modes, const uint32_t* cls, uint8_t* snaps, int* err1, uint32_t* sizes,
                             int* err2, uint32_t* moff, uint64_t* fbase, int* terr, uint64_t* d_total,
                             uint64_t* host_total, int mbw, int mbh, int n, hipEvent_t stage1_done);
hipError_t zwk_dec_tok_write(hipStream_t s, const uint8_t* blob, const ZwTokFrame* tf, const uint8_t* probs,
                             const uint8_t* modes, const uint8_t* snaps, const int* err1, const uint32_t* moff,
                             const uint64_t* fbase, uint8_t* recs, int nmb, int n);
size_t zw_tok1_lds_bytes(int mbw);
size_t zw_alpha_plane_stride(size_t w, size_t h);
hipError_t zwk_alpha_unfilter(hipStream_t s, uint8_t* planes, size_t pstride, int w, int h, int filter,
                              const uint32_t* list, int count);
hipError_t zwk_alpha_store(hipStream_t s, const uint8_t* planes, size_t pstride, const ZwAlphaFrame* tab, int w, int h,
                           int layout, int dtype, void* out, const ZwY2rDev* P, int nframes);
}
// zw_vp8l_host.cpp: a run of lossless files into the caller's tensor
int zw_ll_decode_run(zw_ctx* ctx, int n, const uint8_t* const* payload, const size_t* plen, const uint8_t* has_alpha,
                     uint32_t w, uint32_t h, const ZwLlOut& O);
#include "zw_tokl.h"

using namespace zwdec;

namespace {

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// Decoded frame buffers (zw_frame.y, and decode_rgb_batch's zw_bytes) are
// recycled.  A fresh multi-MB malloc is first touched by the fan-out's copy,
// so each of its 4 KB pages faults and is zeroed by the kernel, on the same
// host threads the bool decoder needs (1024 1080p frames on the box: 4 474-
// 5 022 decodes/s with fresh buffers, 5 132-5 221 recycled).  zw_frame_free /
// zw_bytes_free hand a buffer back to this process-wide pool (keyed by size,
// bounded by ZW_DEC_POOL_MB, default 4096; 0 = off) and the next batch of that
// size takes it.  Only while a context is alive: the last zw_ctx_destroy (and
// every zw_ctx_release_buffers) frees what the pool holds, and buffers freed
// after that go straight back to free().  Buffers the pool handed out are tracked, so zw_bytes_free
// still free()s the encoder's outputs.  (bench decode_path, 1024 1080p
// frames: fan-out 96 -> 67 ms, 5 013 -> 5 289 decodes/s.)
struct FramePool {
    std::mutex m;
    std::unordered_map<size_t, std::vector<uint8_t*>> free_;
    std::unordered_map<uint8_t*, size_t> live;
    size_t bytes = 0, cap = 0;
    FramePool()
    {
        const char* e = getenv("ZW_DEC_POOL_MB");
        cap = (size_t)(e ? std::max(0L, atol(e)) : 4096L) << 20;
    }
    uint8_t* get(size_t n)
    {
        std::lock_guard<std::mutex> g(m);
        uint8_t* p = nullptr;
        auto it = free_.find(n);
        if (it != free_.end() && !it->second.empty()) {
            p = it->second.back();
            it->second.pop_back();
            bytes -= n;
        } else {
            p = (uint8_t*)malloc(n);
            if (!p) return nullptr;
        }
        live[p] = n;
        return p;
    }
    // frees every buffer the pool holds (those handed out stay tracked)
    void trim()
    {
        std::vector<uint8_t*> drop;
        {
            std::lock_guard<std::mutex> g(m);
            for (auto& kv : free_)
                for (uint8_t* b : kv.second) drop.push_back(b);
            free_.clear();
            bytes = 0;
        }
        for (uint8_t* b : drop) free(b);
    }
    // false: p did not come from the pool.  Over the cap, buffers of other
    // sizes are dropped first (the latest frame size is the one reused).
    bool put(void* q)
    {
        uint8_t* p = (uint8_t*)q;
        std::vector<uint8_t*> drop;
        {
            std::lock_guard<std::mutex> g(m);
            auto it = live.find(p);
            if (it == live.end()) return false;
            const size_t n = it->second;
            live.erase(it);
            if (!zw_ctx_any_alive()) {
                free(p);
                return true;
            }
            for (auto& kv : free_) {
                while (bytes + n > cap && kv.first != n && !kv.second.empty()) {
                    drop.push_back(kv.second.back());
                    kv.second.pop_back();
                    bytes -= kv.first;
                }
            }
            if (bytes + n <= cap) {
                free_[n].push_back(p);
                bytes += n;
                p = nullptr;
            }
        }
        for (uint8_t* d : drop) free(d);
        free(p);
        return true;
    }
};
// never destroyed: Python finalizers may free frames during interpreter exit
static FramePool& frame_pool()
{
    static FramePool* P = new FramePool();
    return *P;
}

}  // namespace

bool zw_dec_pool_put(void* p) { return frame_pool().put(p); }
void zw_dec_pool_trim() { frame_pool().trim(); }

extern "C" void zw_frame_free(zw_frame* f)
{
    if (f && f->y) {
        if (!frame_pool().put(f->y)) free(f->y);
        f->y = f->u = f->v = nullptr;
    }
}

namespace {

static double dec_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The decode paths' environment knobs, read once at the top of each call (the
// tests change them between calls in one process: none is cached).
struct DecKnobs {
    // ZW_DEC_CHUNK: frames per pipelined chunk.
    int chunk = 128;  // measured on 256 1080p frames: 32 / 64 / 128 / 256 -> 3198 / 3559 / 3771 / 3267 per s
    // ZW_DEC_DEV_CHUNK: device-parsed frames per chunk.  Their records are all
    // ready at once when the device parse ends, so fewer, longer chunks download
    // back to back behind it (1 024 1080p frames: the tail after the device
    // parse 68 -> ~45 ms)
    int dev_chunk = 512;
    // ZW_DEC_DL_PARTS: parts a chunk's plane download is split into, each fanned
    // out while the next lands.
    int dl_parts = 4;  // 1024 1080p frames: 4 901 vs 4 724 decodes/s with one part
    // ZW_DEC_FAN_THREADS: threads of a fan-out part (0 = every host thread).  The
    // copies into recycled buffers run beside the next chunk's parse; capping them
    // did not help it (1 024 1080p frames: all 16 threads 5 061-5 120 decodes/s,
    // 8: 5 018-5 107, 4: 4 753-4 873; profiles/r04_dec_fan_ab.txt).
    int fan_threads = 0;
    // ZW_DEC_ROWS: 0 / nonzero forces the workgroup-per-frame / the row-parallel
    // kernels (unset, -1: by batch size, dec_launch).
    int rows = -1;
    // ZW_DEC_TOKENS=host / device / mixed forces the host, the device or a split
    // at ZW_DEC_TOKENS_HOST (the host's share, 0.5); anything else: auto (dec_tok_split).
    enum Tokens { TOK_AUTO, TOK_HOST, TOK_DEVICE, TOK_MIXED } tokens = TOK_AUTO;
    double tokens_host = 0.5;
    bool timing = false;                // ZW_DEC_TIMING: per-chunk times on stderr
    bool trace = false;                 // ZW_DEC_TRACE: the chunk timeline (ms from the batch start) on stderr
    const char* tokens_dump = nullptr;  // ZW_DEC_TOKENS_DUMP (debug): frame 0's records to <dump>.host / <dump>.dev
    // ZW_DEC_FORCE_ERROR (test hook): pre-set frame 0's row-sync error word, as a
    // wave that gave up waiting would, so the host-side check is exercised.
    bool force_error = false;

    DecKnobs()
    {
        auto positive = [](const char* name, int dflt) {
            const char* e = getenv(name);
            const int v = e ? atoi(e) : dflt;
            return v > 0 ? v : dflt;
        };
        chunk = positive("ZW_DEC_CHUNK", chunk);
        dev_chunk = positive("ZW_DEC_DEV_CHUNK", dev_chunk);
        dl_parts = positive("ZW_DEC_DL_PARTS", dl_parts);
        if (const char* e = getenv("ZW_DEC_FAN_THREADS")) fan_threads = std::max(0, atoi(e));
        if (const char* e = getenv("ZW_DEC_ROWS")) rows = atoi(e);
        if (const char* e = getenv("ZW_DEC_TOKENS"))
            tokens = !strcmp(e, "device") ? TOK_DEVICE : (!strcmp(e, "host") ? TOK_HOST : (!strcmp(e, "mixed") ? TOK_MIXED : TOK_AUTO));
        if (const char* e = getenv("ZW_DEC_TOKENS_HOST")) tokens_host = atof(e);
        timing = getenv("ZW_DEC_TIMING") != nullptr;
        trace = getenv("ZW_DEC_TRACE") != nullptr;
        tokens_dump = getenv("ZW_DEC_TOKENS_DUMP");
        force_error = getenv("ZW_DEC_FORCE_ERROR") != nullptr;
    }
};

// Where everything of n frames of mbw x mbh MBs lies in a buffer set's device
// scratch (byte offsets, 256-B aligned): the uploaded records (`up_bytes`: the
// packed records, MB offsets and frame bases of a host-parsed chunk), the
// quantisers, the filter tables, the per-MB filter flags, the planes, the
// row-parallel kernels' sync words and borders or the batch kernels' recon ->
// filter MB tiles, then `extra_bytes` for the caller.
struct DecLayout {
    size_t mbs = 0, quant = 0, fparams = 0, flags = 0, y = 0, u = 0, v = 0, rowsync = 0, borders = 0, tiles = 0, extra = 0;
    size_t total = 0;
};
static DecLayout dec_layout(int n, int mbw, int mbh, bool rows, size_t up_bytes, size_t extra_bytes)
{
    const size_t N = (size_t)n, nmb = (size_t)mbw * mbh, ysz = nmb * 256, csz = nmb * 64;
    DecLayout L;
    L.quant = al256(L.mbs + up_bytes);
    L.fparams = al256(L.quant + N * 4 * sizeof(DecQuant));
    L.flags = al256(L.fparams + N * sizeof(ZwFilterParams));
    L.y = al256(L.flags + N * nmb * 4);
    L.u = al256(L.y + N * ysz);
    L.v = al256(L.u + N * csz);
    L.rowsync = al256(L.v + N * csz);
    L.borders = al256(L.rowsync + (rows ? zw_dec_rows_sync_bytes(mbh, n) : 0));
    L.tiles = al256(L.borders + (rows ? zw_dec_rows_border_bytes(mbw, n) : 0));
    L.extra = al256(L.tiles + (rows ? 0 : N * nmb * 384));
    L.total = al256(L.extra + extra_bytes);
    return L;
}

// What the frames of a chunk are: headers, quantisers and filter tables.
struct DecMeta {
    std::vector<DecFrame> F;
    std::vector<DecQuant> quant;       // four per frame
    std::vector<ZwFilterParams> fps;   // one per frame
    int n = 0, mbw = 0, mbh = 0;
    size_t ysz = 0, csz = 0;           // bytes of a frame's luma / one chroma plane (whole MBs)
    double parse_ms = 0;               // the host parse (0 for a device-parsed chunk)
    size_t rec_bytes = 0;              // host-parsed records (for ZW_DEC_TIMING)

    void shape(int frames, int w_mbs, int h_mbs)
    {
        n = frames;
        mbw = w_mbs;
        mbh = h_mbs;
        ysz = (size_t)mbw * mbh * 256;
        csz = (size_t)mbw * mbh * 64;
    }
};

// Where a chunk's packed MB records are.
struct DecRecords {
    // host-staged (dec_parse): one upload of the records, then the MB offsets
    // (at o_moff) and the frame bases (at o_base) from pinned staging
    const uint8_t* stage = nullptr;
    size_t up_bytes = 0, o_moff = 0, o_base = 0;
    // device-resident (dec_parse_dev): the device token parse's output, complete
    // at `done`; `err` = its per-frame error words
    const uint8_t* recs = nullptr;
    const uint32_t* moff = nullptr;
    const uint64_t* fbase = nullptr;
    hipEvent_t done = nullptr;
    const int* err = nullptr;
    bool on_device() const { return recs != nullptr; }
};

// One chunk of a batch in flight: frames [first, first + meta.n) of the run on
// one of the context's two buffer sets.
struct DecChunk {
    int first = 0;
    zw_ctx::DecSet* set = nullptr;
    DecMeta meta;
    DecRecords src;
    // set by dec_launch: the decoded planes, resident in the set's device scratch
    uint8_t* d = nullptr;
    DecLayout lay;
    const int* d_rs = nullptr;  // row-parallel kernels' per-frame sync words (null: workgroup-per-frame kernels)
};

// A parsed frame's four segment quantisers and its filter table, as the kernels read them.
static void frame_tables(const DecFrame& F, DecQuant* quant, ZwFilterParams& fp)
{
    for (int s = 0; s < 4; s++) quant[s] = F.q[s];
    filter_table(fp, F.filter_type, F.filter_level, F.sharpness, F.segments_enabled, F.seg_delta_values, F.seg_lf,
                 F.lf_adj_enabled, F.ref_delta0, F.mode_delta0, F.mbw, F.mbh);
}

// ZW_DEC_TOKENS_DUMP (debug): one frame's MB offsets and records to <dump><suffix>.
static void dump_records(const char* dump, const char* suffix, const uint32_t* moff, size_t nmb, const uint8_t* recs)
{
    if (FILE* fo = fopen((std::string(dump) + suffix).c_str(), "wb")) {
        fwrite(moff, 4, nmb + 1, fo);
        fwrite(recs, 1, moff[nmb], fo);
        fclose(fo);
    }
}

// A row-parallel wave that gives up waiting (k_dec_recon_rows / k_loopfilter_rows
// bounded spins) reports through its frame's error word rowsync[f][2] instead of
// hanging the GPU; the planes of such a frame are incomplete.  Read the words
// after the kernels completed (SDMA: the kernel stream may already run the next
// chunk) and fail the call with ZW_EDEVICE.
static int tokens_error(zw_ctx* ctx, const int* d_terr, int n)
{
    if (!d_terr) return ZW_OK;
    int* e = (int*)ctx->pin[PIN_ERR_WORDS].reserve((size_t)n * sizeof(int));
    if (!e) return ZW_ENOMEM;
    if (int r = ctx_d2h(ctx, e, d_terr, (size_t)n * sizeof(int))) return r;
    for (int f = 0; f < n; f++) {
        if (e[f] == 1) return ZW_EBITSTREAM;  // a token partition ran out (parse_mbs: read_levels_into < 0)
        if (e[f]) {
            fprintf(stderr, "zwebp: device token parse gave up waiting on frame %d of %d\n", f, n);
            return ZW_EDEVICE;
        }
    }
    return ZW_OK;
}

static int rows_error(zw_ctx* ctx, const int* d_rs, int n, int mbh)
{
    if (!d_rs) return ZW_OK;
    const size_t words = (size_t)n * (4 + 2 * mbh);
    int* rs = (int*)ctx->pin[PIN_ERR_WORDS].reserve(words * sizeof(int));
    if (!rs) return ZW_ENOMEM;
    if (int r = ctx_d2h(ctx, rs, d_rs, words * sizeof(int))) return r;
    for (int f = 0; f < n; f++)
        if (rs[(size_t)f * (4 + 2 * mbh) + 2]) {
            fprintf(stderr, "zwebp: row-parallel decode gave up waiting on frame %d of %d\n", f, n);
            return ZW_EDEVICE;
        }
    return ZW_OK;
}

// Vp8Decoder::decode_frame for n frames of identical dimensions, one device
// pass: host header/token parse (parallel over frames, dec_parse) ->
// k_dec_recon -> k_loopfilter (dec_launch).
//
// Host half: headers, modes and tokens of n frames into packed MB records in
// the pinned upload staging of C's buffer set (no device work).
static int dec_parse(int n, const uint8_t* const* data, const size_t* lens, DecChunk& C)
{
    const double t0 = dec_now_ms();
    DecMeta& M = C.meta;
    C.src = DecRecords();
    M.parse_ms = 0;
    M.F.assign(n, DecFrame());
    std::vector<DecFrame>& F = M.F;
    std::vector<int> rc(n, ZW_OK);
    parallel_for(n, [&](int i) { rc[i] = parse_header(F[i], data[i], lens[i]); });
    for (int i = 0; i < n; i++)
        if (rc[i] != ZW_OK) return rc[i];
    const int mbw = F[0].mbw, mbh = F[0].mbh;
    for (int i = 1; i < n; i++)
        if (F[i].mbw != mbw || F[i].mbh != mbh) return ZW_EINVAL;
    if (mbw == 0 || mbh == 0) return ZW_EINVALID_DIMENSIONS;
    M.shape(n, mbw, mbh);
    const size_t nmb = (size_t)mbw * mbh;
    // packed MB records (zw_common.h ZW_DREC_*): each frame is parsed into its
    // own worst-case pageable buffer (only the pages written are touched), then
    // the used prefixes are packed back to back (256-B aligned frame bases) into
    // pinned staging sized by the measured bytes -- ~1 MB per 1080p frame at
    // Q75 instead of the 7 MB worst case -- followed by the MB offsets and the
    // frame bases; one upload carries all of it.
    const size_t slot = nmb * ZW_DREC_MAX;
    std::vector<uint32_t> moffv((size_t)n * (nmb + 1));
    std::vector<zw_ctx::RecBuf>& recs = C.set->recs;
    if (recs.size() < (size_t)n) recs.resize(n);
    M.quant.assign((size_t)n * 4, DecQuant());
    M.fps.assign(n, ZwFilterParams());
    parallel_for(n, [&](int i) {
        if (recs[i].cap < slot) {
            recs[i].p.reset(new (std::nothrow) uint8_t[slot]);
            recs[i].cap = recs[i].p ? slot : 0;
            if (!recs[i].p) {
                rc[i] = ZW_ENOMEM;
                return;
            }
        }
        rc[i] = parse_mbs(F[i], recs[i].p.get(), moffv.data() + (size_t)i * (nmb + 1));
        frame_tables(F[i], &M.quant[(size_t)i * 4], M.fps[i]);
    });
    for (int i = 0; i < n; i++)
        if (rc[i] != ZW_OK) return rc[i];
    std::vector<uint64_t> fb(n);
    size_t rec_span = 0;
    M.rec_bytes = 0;
    for (int i = 0; i < n; i++) {
        fb[i] = rec_span;
        const size_t used = moffv[(size_t)i * (nmb + 1) + nmb];
        M.rec_bytes += used;
        rec_span = al256(rec_span + used);
    }
    const size_t off_bytes = (size_t)n * (nmb + 1) * 4, base_bytes = (size_t)n * 8;
    DecRecords& R = C.src;
    R.o_moff = rec_span;
    R.o_base = R.o_moff + al256(off_bytes);
    R.up_bytes = R.o_base + base_bytes;
    uint8_t* stage = (uint8_t*)C.set->upload.reserve(R.up_bytes);
    if (!stage) return ZW_ENOMEM;
    parallel_for(n, [&](int i) {
        memcpy(stage + fb[i], recs[i].p.get(), moffv[(size_t)i * (nmb + 1) + nmb]);
    });
    memcpy(stage + R.o_moff, moffv.data(), off_bytes);
    memcpy(stage + R.o_base, fb.data(), base_bytes);
    R.stage = stage;
    M.parse_ms = dec_now_ms() - t0;
    return ZW_OK;
}

// Device half: upload the chunk's records (or wait for the device parse's),
// reconstruct, filter.  Leaves the filtered planes in the set's device scratch
// (plus `extra_bytes` of scratch at lay.extra for the caller) with the kernel
// stream's work queued; the set's DEC_EV_FILTER_DONE marks the end of the loop filter.
static int dec_launch(zw_ctx* ctx, const DecKnobs& K, size_t extra_bytes, DecChunk& C)
{
    const double t1 = dec_now_ms();
    const DecMeta& M = C.meta;
    const DecRecords& R = C.src;
    const int n = M.n, mbw = M.mbw, mbh = M.mbh;
    HIPOK(hipSetDevice(ctx->device));
    // Small batches run the row-parallel kernels (one wave per MB row, the x+2y
    // wavefront spread over up to mbh CUs); large ones fill the GPU with one
    // workgroup per frame.  ZW_DEC_ROWS=0/1 forces either.
    const bool rows = K.rows >= 0 ? K.rows != 0 : n < 128;  // measured: rows faster up to 64, slower at 256
    const DecLayout L = dec_layout(n, mbw, mbh, rows, R.up_bytes, extra_bytes);
    uint8_t* d = (uint8_t*)C.set->scratch.reserve(L.total);
    if (!d) return ZW_ENOMEM;
    hipStream_t s = ctx_stream(ctx);
    hipEvent_t* ev = C.set->ev;
    if (R.up_bytes) HIPOK(hipMemcpyAsync(d + L.mbs, R.stage, R.up_bytes, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.quant, M.quant.data(), M.quant.size() * sizeof(DecQuant), hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.fparams, M.fps.data(), M.fps.size() * sizeof(ZwFilterParams), hipMemcpyHostToDevice, s));
    for (int e = 0; e < DEC_EV_COUNT; e++)  // blocking sync: the finisher sleeps on them (ctx_d2h_stream)
        if (!ev[e]) HIPOK(hipEventCreateWithFlags(&ev[e], hipEventBlockingSync));
    // the kernels read the packed records straight from the upload, or, for a
    // chunk whose tokens the device parsed, from k_dec_tokl's output
    const uint8_t* recs = d + L.mbs;
    const uint32_t* moff = (const uint32_t*)(d + L.mbs + R.o_moff);
    const uint64_t* fbase = (const uint64_t*)(d + L.mbs + R.o_base);
    if (R.on_device()) {
        HIPOK(hipStreamWaitEvent(s, R.done, 0));
        recs = R.recs;
        moff = R.moff;
        fbase = R.fbase;
    } else if (K.tokens_dump) {  // frame 0's host records
        dump_records(K.tokens_dump, ".host", (const uint32_t*)(R.stage + R.o_moff), (size_t)mbw * mbh, R.stage);
    }
    uint8_t *Y = d + L.y, *U = d + L.u, *V = d + L.v, *flags = d + L.flags;
    const ZwFilterParams* fp = (const ZwFilterParams*)(d + L.fparams);
    HIPOK(hipEventRecord(ev[DEC_EV_RECON_START], s));
    // two wavefront kernels (a fused recon + filter wavefront measured slower: the
    // per-MB latencies add up in one chain, and its registers spilled)
    if (rows) {
        int* rs = (int*)(d + L.rowsync);
        HIPOK(zwk_dec_rows_init(s, rs, mbh, n));
        if (K.force_error) HIPOK(hipMemsetAsync(rs + 2, 1, sizeof(int), s));
        HIPOK(zwk_dec_rows(s, 1, recs, moff, fbase, d + L.quant, Y, U, V, flags, fp, mbw, mbh, M.ysz, M.csz, n, rs,
                           d + L.borders, mbh));
        HIPOK(hipEventRecord(ev[DEC_EV_RECON_DONE], s));
        HIPOK(zwk_dec_rows(s, 2, nullptr, nullptr, nullptr, d + L.quant, Y, U, V, flags, fp, mbw, mbh, M.ysz, M.csz, n,
                           rs, d + L.borders, mbh));
    } else {
        HIPOK(zwk_dec_recon(s, recs, moff, fbase, d + L.quant, Y, U, V, flags, mbw, mbh, M.ysz, M.csz, n, d + L.tiles));
        HIPOK(hipEventRecord(ev[DEC_EV_RECON_DONE], s));
        HIPOK(zwk_loopfilter(s, Y, U, V, flags, fp, M.ysz, M.csz, n, mbw, d + L.tiles));
    }
    HIPOK(hipEventRecord(ev[DEC_EV_FILTER_DONE], s));
    if (K.timing) {
        HIPOK(hipEventSynchronize(ev[DEC_EV_FILTER_DONE]));
        fprintf(stderr, "[dec] n=%d parse %.2f ms, upload+kernels %.2f ms (records %.1f MB)\n", n, M.parse_ms,
                dec_now_ms() - t1, M.rec_bytes / 1e6);
    }
    C.d = d;
    C.lay = L;
    C.d_rs = rows ? (const int*)(d + L.rowsync) : nullptr;
    return ZW_OK;
}

// Where a batch's decoded frames go: the planes of zw_vp8_decode_batch or the
// packed RGB(A) images of the RGB entries.  The chunk pipeline (DecRun) drives it.
struct DecSink {
    virtual ~DecSink() {}
    // device scratch the sink needs per frame beside the planes (at lay.extra)
    virtual size_t extra_per_frame() const = 0;
    // host work of the sink's own for the chunk's frames [first, first + cnt),
    // started before the chunk's device work is queued (set 0 / 1 = the buffer
    // set the chunk runs on); enqueue collects it
    virtual void begin_chunk(zw_ctx*, int /*first*/, int /*cnt*/, int /*set*/) {}
    // checks the chunk and queues the sink's device work after the loop filter
    virtual int enqueue(zw_ctx* ctx, DecChunk& C) = 0;
    // the set's event that marks the chunk's device work done
    virtual DecEv wait_event() const = 0;
    // pinned download staging per frame; 0: the frames stay on the device, and
    // the chunk has nothing to bring down (copy_down / place are not called)
    virtual size_t staging_per_frame(const DecChunk& C) const = 0;
    // the chunk's frames [a, b) from the device into the staging `hout`
    virtual int copy_down(zw_ctx* ctx, const DecChunk& C, uint8_t* hout, int a, int b) = 0;
    // the chunk's frame i from the staging to the caller; false: out of memory
    virtual bool place(const DecChunk& C, const uint8_t* hout, int i) = 0;
};

// A chunk's download in parts on a second thread, each part (frames [a, b))
// placed as soon as copy_down has landed it, so the fan-out into the callers'
// buffers overlaps the rest of the download.  Returns the first copy error;
// *dl_ms = the download's wall time; oom[i] = frame i could not be placed.
static int dec_download_fan(zw_ctx* ctx, const DecKnobs& K, DecSink& sink, const DecChunk& C, uint8_t* hout,
                            std::vector<int>& oom, double* dl_ms)
{
    const int cn = C.meta.n, parts = std::max(1, std::min(cn, K.dl_parts));
    Progress parts_down;
    int err = ZW_OK;  // the downloader's, read after the join
    const double t0 = dec_now_ms();
    std::thread dl([&]() {
        (void)hipSetDevice(ctx->device);
        for (int p = 0; p < parts; p++) {
            err = sink.copy_down(ctx, C, hout, cn * p / parts, cn * (p + 1) / parts);
            if (err) {
                parts_down.stop();
                break;
            }
            parts_down.advance();
        }
        *dl_ms = dec_now_ms() - t0;
    });
    // the waiting thread sleeps (a spinning one took a CPU from the parse threads)
    for (int p = 0; p < parts && parts_down.wait_for(p + 1); p++) {
        const int a = cn * p / parts, b = cn * (p + 1) / parts;
        parallel_for(b - a, [&](int k) {
            if (!sink.place(C, hout, a + k)) oom[a + k] = 1;
        }, K.fan_threads);
    }
    dl.join();
    return err;
}

// ---------------------------------------------------------------------------
// Device token parse (zw_dec_tokens.hip) for the tail of a batch.  A frame's
// token partition is one serial chain of bool decisions: ≈2.7 ms on a host core
// for a 1080p Q75 frame, much longer on one GPU lane, but one launch runs 64
// frames per wave side by side, so its time hardly depends on how many frames it
// holds.  So a batch splits: the frames [h0, n) are header/mode-parsed on the
// host up front (the first partition, a short chain) and their tokens go to the
// device on its own stream, while the chunk pipeline parses the frames [0, h0)
// on the host as before; the device chunks' reconstruction waits for the
// device's records.  The device parse runs in two stages: k_dec_tok1 (the
// decision chains alone, a snapshot per MB) and k_dec_tok2 (every MB replayed
// from its snapshot in parallel: a count pass, offsets, then the records into a
// buffer sized from the count, so the records take what they use -- ≈1 MB per
// 1080p Q75 frame -- and no worst-case slots).  By default (auto) the host keeps
// as many whole chunks as it parses in the device's time, from the rates the
// last batches measured, and the device takes the rest (none when the host
// alone would finish first).  ZW_DEC_TOKENS=host / device / mixed forces the
// host, the device or a split at ZW_DEC_TOKENS_HOST (the host's share, 0.5).
//
// Device memory the parse keeps in the context after a batch (freed by
// zw_ctx_release_buffers / zw_ctx_destroy; grow-only between): per device frame
// its partition, modes (16 B per MB), probabilities, a 16-byte snapshot and a
// 4-byte size and offset per MB (≈0.4 MB per 1080p frame) plus its records.
// ---------------------------------------------------------------------------

// The parse's upload, as staged in pinned memory and as it lies at the start of
// its device buffer: per frame the modes, the MB class words (2 bits per MB: I4,
// skipped), the probabilities and the ZwTokFrame, then the token partitions
// (16-byte aligned, 16 zero bytes at the end).
struct TokUpload {
    size_t modes = 0, cls = 0, probs = 0, frames = 0, blob = 0, bytes = 0;
};
static TokUpload tok_upload_layout(int nd, size_t nmb, size_t blob_bytes)
{
    const size_t N = (size_t)nd, ncw = (nmb + 15) / 16;
    TokUpload u;
    u.cls = al256(u.modes + N * nmb * ZW_TOK_MODE);
    u.probs = al256(u.cls + N * ncw * 4);
    u.frames = al256(u.probs + N * (size_t)tokl::PROBS);
    u.blob = al256(u.frames + N * sizeof(ZwTokFrame));
    u.bytes = al256(u.blob + blob_bytes);
    return u;
}

// What the parse's kernels write behind the upload in the device buffer: stage
// 1's snapshots and error words, the count pass's sizes and error words, the MB
// offsets, the frame bases, the per-frame error words the host reads and the
// total.
struct TokWork {
    size_t snaps = 0, sizes = 0, moff = 0, fbase = 0, err1 = 0, err2 = 0, terr = 0, total_word = 0, bytes = 0;
};
static TokWork tok_work_layout(int nd, size_t nmb, size_t up_bytes)
{
    const size_t N = (size_t)nd;
    TokWork w;
    w.snaps = up_bytes;
    w.sizes = al256(w.snaps + N * nmb * 16);
    w.moff = al256(w.sizes + N * nmb * 4);
    w.fbase = al256(w.moff + N * (nmb + 1) * 4);
    w.err1 = al256(w.fbase + N * 8);
    w.err2 = al256(w.err1 + N * 4);
    w.terr = al256(w.err2 + N * 4);
    w.total_word = al256(w.terr + N * 4);
    w.bytes = al256(w.total_word + 8);
    return w;
}

struct DecTok {
    int h0 = 0, nd = 0;  // device frames [h0, h0 + nd)
    std::vector<DecFrame> F;
    std::vector<DecQuant> quant;
    std::vector<ZwFilterParams> fps;
    size_t nmb = 0;
    // the device buffer of the count and record passes (ctx->tok_scratch)
    uint8_t* d = nullptr;
    TokUpload up;
    TokWork work;
    const uint32_t* moff() const { return (const uint32_t*)(d + work.moff); }
    const uint64_t* fbase() const { return (const uint64_t*)(d + work.fbase); }
    const int* err() const { return (const int*)(d + work.terr); }
    // set by dec_tok_finish
    const uint8_t* recs = nullptr;
    hipEvent_t done = nullptr;
    // LAUNCHED: stage 1 and the count pass are queued; FAILED: the host parses the rest
    enum State { LAUNCHED, RECORDS_QUEUED, FAILED } state = LAUNCHED;
};

// The host's frames [0, h0) of a batch of n frames of nmb MBs (C frames per chunk).
static int dec_tok_split(zw_ctx* ctx, const DecKnobs& K, int n, size_t nmb)
{
    const int C = K.chunk;
    if (K.tokens == DecKnobs::TOK_HOST) return n;
    if (K.tokens == DecKnobs::TOK_DEVICE) return 0;
    if (K.tokens == DecKnobs::TOK_MIXED) return std::max(0, std::min(n, (int)(n * K.tokens_host) / C * C));  // whole host chunks
    // auto.  Defaults until measured: 0.19 ms of chunk time per 1080p frame (16 host
    // threads) and a 100 ms device parse for 1080p frames
    const double host_f = (ctx->dec_host_ms_per_mb > 0 ? ctx->dec_host_ms_per_mb : 0.19 / 8160.0) * (double)nmb;
    const double tok = (ctx->dec_tok_ms_per_mb > 0 ? ctx->dec_tok_ms_per_mb : 100.0 / 8160.0) * (double)nmb;
    const double tail = 0.06 * tok;  // the device frames' reconstruction and download after the parse, per frame of
                                     // host work that the parse's length leaves (an estimate; errs toward the host)
    if (n * host_f <= tok + tail) return n;  // the host alone finishes first
    const int h0 = (int)(tok / host_f) / C * C;
    return std::max(0, std::min(n, h0));
}

// Parses the headers and modes of frames [h0, n), stages them and launches the
// device parse's first half (stage 1, the count pass, offsets) on the context's
// token stream.  Returns false (and leaves the frames to the host chunks, which
// then report any error in frame order) when a frame has several token
// partitions, another size, or a header / mode error.
static bool dec_tok_prepare(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, int h0, DecTok& T)
{
    const int nd = n - h0;
    if (nd <= 0) return false;
    T.F.assign(nd, DecFrame());
    std::vector<DecFrame>& F = T.F;
    std::vector<int> rc(nd, ZW_OK);
    parallel_for(nd, [&](int i) { rc[i] = parse_header(F[i], data[h0 + i], lens[h0 + i]); });
    for (int i = 0; i < nd; i++)
        if (rc[i] != ZW_OK || F[i].nparts != 1 || F[i].mbw != F[0].mbw || F[i].mbh != F[0].mbh || F[i].mbw == 0 ||
            F[i].mbh == 0)
            return false;
    const int mbw = F[0].mbw, mbh = F[0].mbh;
    // stage 1 keeps per-lane top contexts in LDS (very wide frames stay on the host) and
    // addresses a wave's 64 frames of snapshots through one buffer (< 2 GB)
    const size_t nmb = (size_t)mbw * mbh, ncw = (nmb + 15) / 16;
    if (mbw < 2 || zw_tok1_lds_bytes(mbw) > 160 * 1024 || 64 * nmb * 16 >= ((size_t)1 << 31)) return false;
    std::vector<size_t> boff(nd);
    size_t blob = 0;
    for (int i = 0; i < nd; i++) {
        boff[i] = blob;
        blob += (F[i].part[0].len + 15) & ~(size_t)15;
    }
    blob += 16;  // (16 zero bytes at the end)
    const TokUpload up = tok_upload_layout(nd, nmb, blob);
    uint8_t* stage = (uint8_t*)ctx->pin[PIN_TOK_UPLOAD].reserve(up.bytes);
    if (!stage) return false;
    T.quant.assign((size_t)nd * 4, DecQuant());
    T.fps.assign(nd, ZwFilterParams());
    parallel_for(nd, [&](int i) {
        uint8_t* mr = stage + up.modes + (size_t)i * nmb * ZW_TOK_MODE;
        rc[i] = parse_modes(F[i], mr);
        uint32_t* cw = (uint32_t*)(stage + up.cls) + (size_t)i * ncw;  // 2 bits per MB: I4, skipped
        memset(cw, 0, ncw * 4);
        for (size_t j = 0; j < nmb; j++) {
            const uint8_t b0 = mr[j * ZW_TOK_MODE];
            cw[j >> 4] |= ((uint32_t)((b0 & 7) == 4) | (uint32_t)((b0 >> 5) & 1) << 1) << (2 * (j & 15));
        }
        memcpy(stage + up.probs + (size_t)i * tokl::PROBS, F[i].probs, tokl::PROBS);  // [type][band][ctx][node]
        const ZwTokFrame tf = {boff[i], (uint32_t)F[i].part[0].len, 0};
        memcpy(stage + up.frames + (size_t)i * sizeof(ZwTokFrame), &tf, sizeof tf);
        const size_t len = F[i].part[0].len, al = (len + 15) & ~(size_t)15;
        memcpy(stage + up.blob + boff[i], F[i].part[0].d, len);
        memset(stage + up.blob + boff[i] + len, 0, al - len);
        frame_tables(F[i], &T.quant[(size_t)i * 4], T.fps[i]);
    });
    for (int i = 0; i < nd; i++)
        if (rc[i] != ZW_OK) return false;
    memset(stage + up.blob + blob - 16, 0, 16);
    const TokWork w = tok_work_layout(nd, nmb, up.bytes);
    uint8_t* d = (uint8_t*)ctx->tok_scratch.reserve(w.bytes);
    if (!d) return false;
    if (!ctx->tok_total && hipHostMalloc((void**)&ctx->tok_total, 256, hipHostMallocDefault) != hipSuccess) {
        ctx->tok_total = nullptr;
        return false;
    }
    if (!ctx->tok_ && hipStreamCreateWithFlags(&ctx->tok_, hipStreamNonBlocking) != hipSuccess) return false;
    for (hipEvent_t& e : ctx->tok_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return false;
    hipStream_t s = ctx->tok_;
    if (hipMemcpyAsync(d, stage, up.bytes, hipMemcpyHostToDevice, s) != hipSuccess) return false;
    if (hipEventRecord(ctx->tok_ev[TOK_EV_START], s) != hipSuccess) return false;
    if (zwk_dec_tok_count(s, d + up.blob, (const ZwTokFrame*)(d + up.frames), d + up.probs, d + up.modes,
                          (const uint32_t*)(d + up.cls), d + w.snaps, (int*)(d + w.err1), (uint32_t*)(d + w.sizes),
                          (int*)(d + w.err2), (uint32_t*)(d + w.moff), (uint64_t*)(d + w.fbase), (int*)(d + w.terr),
                          (uint64_t*)(d + w.total_word), ctx->tok_total, mbw, mbh, nd,
                          ctx->tok_ev[TOK_EV_STAGE1]) != hipSuccess ||
        hipEventRecord(ctx->tok_ev[TOK_EV_COUNTED], s) != hipSuccess) {
        (void)hipStreamSynchronize(s);  // (work may be in flight: let it finish before the host takes over)
        return false;
    }
    T.h0 = h0;
    T.nd = nd;
    T.nmb = nmb;
    T.d = d;
    T.up = up;
    T.work = w;
    T.state = DecTok::LAUNCHED;
    return true;
}

// The device parse's second half, once, before the first device chunk: waits
// for the count (the host thread blocks; the previous chunk's download and
// fan-out run on their own thread meanwhile), sizes the record buffer and
// queues the record pass.  false: the host parses the device frames instead.
static bool dec_tok_finish(zw_ctx* ctx, const DecKnobs& K, DecTok& T)
{
    if (T.state != DecTok::LAUNCHED) return T.state == DecTok::RECORDS_QUEUED;
    T.state = DecTok::FAILED;
    if (hipEventSynchronize(ctx->tok_ev[TOK_EV_COUNTED]) != hipSuccess) return false;
    const size_t bytes = std::max<size_t>(256, (size_t)*ctx->tok_total);
    uint8_t* recs = (uint8_t*)ctx->tok_recs.reserve(bytes);
    if (!recs) return false;
    hipStream_t s = ctx->tok_;
    uint8_t* d = T.d;
    if (zwk_dec_tok_write(s, d + T.up.blob, (const ZwTokFrame*)(d + T.up.frames), d + T.up.probs, d + T.up.modes,
                          d + T.work.snaps, (const int*)(d + T.work.err1), T.moff(), T.fbase(), recs, (int)T.nmb,
                          T.nd) != hipSuccess ||
        hipEventRecord(ctx->tok_ev[TOK_EV_RECORDS], s) != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return false;
    }
    T.recs = recs;
    T.done = ctx->tok_ev[TOK_EV_RECORDS];
    T.state = DecTok::RECORDS_QUEUED;
    if (K.tokens_dump && hipStreamSynchronize(s) == hipSuccess) {  // device frame 0's records
        std::vector<uint32_t> mo(T.nmb + 1);
        uint64_t fb0 = 0;
        (void)hipMemcpy(mo.data(), T.moff(), (T.nmb + 1) * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&fb0, T.fbase(), 8, hipMemcpyDeviceToHost);
        std::vector<uint8_t> dev(mo[T.nmb]);
        (void)hipMemcpy(dev.data(), recs + fb0, mo[T.nmb], hipMemcpyDeviceToHost);
        dump_records(K.tokens_dump, ".dev", mo.data(), T.nmb, dev.data());
    }
    return true;
}

// A chunk of `cnt` device frames from C.first: no host parse; its records are the device parse's.
static void dec_parse_dev(const DecTok& T, int cnt, DecChunk& C)
{
    const int j0 = C.first - T.h0;
    DecMeta& M = C.meta;
    M.F.assign(T.F.begin() + j0, T.F.begin() + j0 + cnt);
    M.quant.assign(T.quant.begin() + (size_t)j0 * 4, T.quant.begin() + (size_t)(j0 + cnt) * 4);
    M.fps.assign(T.fps.begin() + j0, T.fps.begin() + j0 + cnt);
    M.shape(cnt, T.F[0].mbw, T.F[0].mbh);
    M.parse_ms = 0;
    M.rec_bytes = 0;
    C.src = DecRecords();
    C.src.recs = T.recs;
    C.src.moff = T.moff() + (size_t)j0 * (T.nmb + 1);
    C.src.fbase = T.fbase() + j0;
    C.src.done = T.done;
    C.src.err = T.err() + j0;
}

// One run of a batch (n frames of one size) through the chunk pipeline,
// alternating the context's two buffer sets.  Per step c the host parses chunk
// c while a second thread finishes chunk c-1 (waits for its kernels, downloads
// and fans out -- mostly a DMA wait), then chunk c is uploaded and launched;
// the device runs chunk c-1 during both.  One finisher thread per step and one
// downloader thread per chunk (dec_download_fan).  Device times of all chunks
// add up in ctx->dec_ms.
struct DecRun {
    zw_ctx* ctx;
    const int n;
    const uint8_t* const* data;
    const size_t* lens;
    DecSink& sink;
    const DecKnobs K;
    DecTok T;           // the device's share of the tokens
    std::vector<int> cb;  // chunk c = frames [cb[c], cb[c + 1])
    DecChunk B[2];
    double host_parse_ms = 0;
    int host_frames = 0;
    size_t nmb = 0;  // MBs of a frame (from the first frame's dimensions; 0: not known)

    DecRun(zw_ctx* c, int frames, const uint8_t* const* d, const size_t* l, DecSink& s)
        : ctx(c), n(frames), data(d), lens(l), sink(s)
    {
    }
    int chunks() const { return (int)cb.size() - 1; }
    bool device_chunk(int c) const { return c < chunks() && cb[c] >= T.h0; }

    // The device's share of the tokens first (its launch runs beside the host
    // chunks), then the chunks: K.chunk frames while the host parses, then the
    // device-parsed frames in chunks of up to K.dev_chunk.
    void plan_chunks()
    {
        const double t0 = dec_now_ms();
        int w = 0, h = 0;  // (the first frame's dimensions; dec_tok_prepare checks every frame)
        nmb = n > 0 && peek_dims(data[0], lens[0], &w, &h) ? (size_t)((w + 15) / 16) * (size_t)((h + 15) / 16) : 0;
        const int h0 = nmb ? dec_tok_split(ctx, K, n, nmb) : n;
        if (h0 >= n || !dec_tok_prepare(ctx, n, data, lens, h0, T)) T.h0 = n;
        ctx->dec_host_ms[0] += dec_now_ms() - t0;
        for (int f = 0; f < n;) {
            cb.push_back(f);
            f += f < T.h0 ? std::min(K.chunk, T.h0 - f) : K.dev_chunk;
        }
        cb.push_back(n);
    }

    // Chunk c's records and metadata into B[c & 1]: the device parse's, or a host parse.
    int parse_chunk(int c)
    {
        DecChunk& C = B[c & 1];
        const int cnt = cb[c + 1] - cb[c];
        C.first = cb[c];
        C.set = &ctx->set[c & 1];
        int err = ZW_OK;
        if (C.first >= T.h0 && dec_tok_finish(ctx, K, T)) {
            dec_parse_dev(T, cnt, C);
        } else {
            err = dec_parse(cnt, data + C.first, lens + C.first, C);
            host_parse_ms += C.meta.parse_ms;
            host_frames += cnt;
        }
        ctx->dec_host_ms[0] += C.meta.parse_ms;
        return err;
    }

    int launch_chunk(int c)
    {
        DecChunk& C = B[c & 1];
        sink.begin_chunk(ctx, C.first, C.meta.n, c & 1);
        if (int r = dec_launch(ctx, K, sink.extra_per_frame() * C.meta.n, C)) return r;
        return sink.enqueue(ctx, C);
    }

    // Waits for the chunk's device work, checks the kernels' error words, then
    // brings the frames down through pinned staging and fans them out to the
    // caller (nothing for a sink without host staging).  The download and fan-out times are added before the download's
    // status is looked at: they are wall time spent either way.
    int finish_chunk(DecChunk& C)
    {
        const DecMeta& M = C.meta;
        const size_t staging = (size_t)M.n * sink.staging_per_frame(C);
        uint8_t* hout = staging ? (uint8_t*)ctx->pin[PIN_DOWNLOAD].reserve(staging) : nullptr;
        if (staging && !hout) return ZW_ENOMEM;
        HIPOK(hipEventSynchronize(C.set->ev[sink.wait_event()]));
        if (int r = tokens_error(ctx, C.src.err, M.n)) return r;
        if (int r = rows_error(ctx, C.d_rs, M.n, M.mbh)) return r;
        if (staging) {  // (a sink that keeps the frames on the device: no download, no fan-out)
            const double tf = dec_now_ms();
            std::vector<int> oom(M.n, 0);
            double dl_ms = 0;
            const int dr = dec_download_fan(ctx, K, sink, C, hout, oom, &dl_ms);
            ctx->dec_host_ms[1] += dl_ms;
            ctx->dec_host_ms[2] += dec_now_ms() - tf;
            if (K.timing) fprintf(stderr, "[dec] download+fanout %.2f ms\n", dec_now_ms() - tf);
            if (dr) return dr;
            for (int i = 0; i < M.n; i++)
                if (oom[i]) return ZW_ENOMEM;
        }
        float ms = 0.f;
        if (sink.wait_event() == DEC_EV_CALLER &&
            hipEventElapsedTime(&ms, C.set->ev[DEC_EV_FILTER_DONE], C.set->ev[DEC_EV_CALLER]) == hipSuccess)
            ctx->dec_ms[2] += ms;
        return ZW_OK;
    }

    // The device token parse's time and stages, and the rates dec_tok_split reads.
    void collect_token_times(int err)
    {
        if (T.nd > 0) {
            if (T.state == DecTok::LAUNCHED) (void)hipStreamSynchronize(ctx->tok_);  // (an error before the first device chunk)
            const hipEvent_t* ev = ctx->tok_ev;
            float ms = 0.f;
            if (T.state == DecTok::RECORDS_QUEUED && hipEventSynchronize(T.done) == hipSuccess &&
                hipEventElapsedTime(&ms, ev[TOK_EV_START], ev[TOK_EV_RECORDS]) == hipSuccess) {
                ctx->dec_tok_ms = ms;
                float m = 0.f;
                if (hipEventElapsedTime(&m, ev[TOK_EV_START], ev[TOK_EV_STAGE1]) == hipSuccess) ctx->dec_tok_stage_ms[0] = m;
                if (hipEventElapsedTime(&m, ev[TOK_EV_STAGE1], ev[TOK_EV_COUNTED]) == hipSuccess) ctx->dec_tok_stage_ms[1] = m;
                if (hipEventElapsedTime(&m, ev[TOK_EV_COUNTED], ev[TOK_EV_RECORDS]) == hipSuccess) ctx->dec_tok_stage_ms[2] = m;
                if (!err && ms > 0) ctx->dec_tok_ms_per_mb = ms / (double)T.nmb;
            }
        }
        // (a chunk's parse runs while the previous chunk downloads: the chunk time is its share of the pipe)
        if (!err && host_frames >= K.chunk && host_parse_ms > 0 && nmb)
            ctx->dec_host_ms_per_mb = host_parse_ms / host_frames / (double)nmb;
    }

    int run()
    {
        ctx->dec_ms[0] = ctx->dec_ms[1] = ctx->dec_ms[2] = 0.f;
        ctx->dec_tok_ms = 0.f;
        ctx->dec_tok_stage_ms[0] = ctx->dec_tok_stage_ms[1] = ctx->dec_tok_stage_ms[2] = 0.f;
        ctx->dec_host_ms[0] = ctx->dec_host_ms[1] = ctx->dec_host_ms[2] = 0;
        plan_chunks();
        const int nch = chunks();
        int err = ZW_OK;
        const double tb = dec_now_ms();
        for (int c = 0; c <= nch && !err; c++) {
            int err_f = ZW_OK, err_p = ZW_OK;
            std::thread fin;
            double tf0 = 0, tf1 = 0;
            if (c >= 1) {
                fin = std::thread([&, c]() {
                    (void)hipSetDevice(ctx->device);
                    DecChunk& P = B[(c - 1) & 1];
                    tf0 = dec_now_ms() - tb;
                    err_f = finish_chunk(P);
                    tf1 = dec_now_ms() - tb;
                    const hipEvent_t* ev = P.set->ev;
                    float ms = 0.f;
                    if (hipEventElapsedTime(&ms, ev[DEC_EV_RECON_START], ev[DEC_EV_RECON_DONE]) == hipSuccess) ctx->dec_ms[0] += ms;
                    if (hipEventElapsedTime(&ms, ev[DEC_EV_RECON_DONE], ev[DEC_EV_FILTER_DONE]) == hipSuccess) ctx->dec_ms[1] += ms;
                });
            }
            const double tp0 = dec_now_ms() - tb;
            if (c < nch) err_p = parse_chunk(c);
            const double tp1 = dec_now_ms() - tb;
            if (fin.joinable()) fin.join();
            err = err_f ? err_f : err_p;
            if (c < nch && !err) err = launch_chunk(c);
            if (K.trace)
                fprintf(stderr, "[dec trace] c=%d %s parse %.1f-%.1f, finish(c-1) %.1f-%.1f, launched %.1f ms\n", c,
                        device_chunk(c) ? "dev " : "host", tp0, tp1, tf0, tf1, dec_now_ms() - tb);
        }
        collect_token_times(err);
        if (err) (void)hipStreamSynchronize(ctx_stream(ctx));  // nothing queued may outlive the call
        return err;
    }
};

// A batch's frames in runs of one size: each run decodes as a batch of its own
// (the device buffers and the packed images of a run are per size), in frame
// order, so the first failing frame's error is the one returned, as a sequence
// of decode_frame calls (decoder/vp8.rs:1526) would report it.  fn(i0, i1)
// decodes the run [i0, i1) (frames too short for dimensions stand alone); the
// first nonzero result ends the walk and is returned.
template <class FN>
static int for_each_run(int n, const uint8_t* const* data, const size_t* lens, FN&& fn)
{
    auto key = [&](int i) -> uint32_t {
        int w = 0, h = 0;
        if (!peek_dims(data[i], lens[i], &w, &h)) return 0xffffffffu;
        return (uint32_t)w | ((uint32_t)h << 16);
    };
    for (int i0 = 0; i0 < n;) {
        const uint32_t k0 = key(i0);
        int i1 = i0 + 1;
        if (k0 != 0xffffffffu)
            while (i1 < n && key(i1) == k0) i1++;
        if (const int r = fn(i0, i1)) return r;
        i0 = i1;
    }
    return ZW_OK;
}

// zw_vp8_decode_batch's output: the planes down through pinned staging (all the
// chunk's Y planes, then its U, then its V), then fanned out into one buffer
// per frame.
struct PlanesSink : DecSink {
    zw_frame* outs;
    int mbw0 = -1, mbh0 = -1;
    explicit PlanesSink(zw_frame* o) : outs(o) {}
    size_t extra_per_frame() const override { return 0; }
    int enqueue(zw_ctx*, DecChunk& C) override
    {
        if (mbw0 < 0) mbw0 = C.meta.mbw, mbh0 = C.meta.mbh;
        return C.meta.mbw == mbw0 && C.meta.mbh == mbh0 ? ZW_OK : ZW_EINVAL;  // one size per batch, as in one chunk
    }
    DecEv wait_event() const override { return DEC_EV_FILTER_DONE; }
    size_t staging_per_frame(const DecChunk& C) const override { return C.meta.ysz + 2 * C.meta.csz; }
    // three plane copies per frame range
    int copy_down(zw_ctx* ctx, const DecChunk& C, uint8_t* hout, int a, int b) override
    {
        const size_t A = (size_t)a, N = (size_t)(b - a), cn = (size_t)C.meta.n, ysz = C.meta.ysz, csz = C.meta.csz;
        int r = ctx_d2h_stream(ctx, hout + A * ysz, C.d + C.lay.y + A * ysz, N * ysz);
        if (!r) r = ctx_d2h_stream(ctx, hout + cn * ysz + A * csz, C.d + C.lay.u + A * csz, N * csz);
        if (!r) r = ctx_d2h_stream(ctx, hout + cn * (ysz + csz) + A * csz, C.d + C.lay.v + A * csz, N * csz);
        return r;
    }
    bool place(const DecChunk& C, const uint8_t* hout, int i) override
    {
        const DecMeta& M = C.meta;
        const size_t cn = (size_t)M.n, ysz = M.ysz, csz = M.csz;
        uint8_t* buf = frame_pool().get(ysz + 2 * csz);
        if (!buf) return false;
        memcpy(buf, hout + (size_t)i * ysz, ysz);
        memcpy(buf + ysz, hout + cn * ysz + (size_t)i * csz, csz);
        memcpy(buf + ysz + csz, hout + cn * (ysz + csz) + (size_t)i * csz, csz);
        const DecFrame& F = M.F[i];
        zw_frame& o = outs[C.first + i];
        o.width = (uint16_t)F.width;
        o.height = (uint16_t)F.height;
        o.y_stride = (uint32_t)M.mbw * 16;
        o.uv_stride = (uint32_t)M.mbw * 8;
        o.mb_rows = (uint32_t)M.mbh;
        o.y = buf;
        o.u = buf + ysz;
        o.v = buf + ysz + csz;
        o.filter_type = (uint8_t)F.filter_type;
        o.filter_level = (uint8_t)F.filter_level;
        o.sharpness_level = (uint8_t)F.sharpness;
        return true;
    }
};

static int dec_batch_one(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, zw_frame* outs)
{
    for (int i = 0; i < n; i++) memset(&outs[i], 0, sizeof(zw_frame));
    PlanesSink sink(outs);
    const int r = DecRun(ctx, n, data, lens, sink).run();
    if (r)
        for (int k = 0; k < n; k++) zw_frame_free(&outs[k]);
    return r;
}

}  // namespace

extern "C" int zw_vp8_decode_batch(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, zw_frame* outs)
{
    if (!ctx || n <= 0 || !data || !lens || !outs) return ZW_EINVAL;
    for (int i = 0; i < n; i++) memset(&outs[i], 0, sizeof(zw_frame));
    int done = 0;  // frames of the runs already decoded
    const int r = for_each_run(n, data, lens, [&](int i0, int i1) {
        done = i0;
        return dec_batch_one(ctx, i1 - i0, data + i0, lens + i0, outs + i0);
    });
    if (r)
        for (int k = 0; k < done; k++) zw_frame_free(&outs[k]);
    return r;
}

namespace {

// The RGB entries' output: k_yuv2rgb after the filter into the scratch's extra
// area, the packed images down, then each into a new buffer (outs) or the
// caller's buffer (dst[i], rows `stride` bytes apart).
struct RgbSink : DecSink {
    size_t w = 0, h = 0, row = 0, fbytes = 0, stride = 0;
    int bpp = 0, fancy = 0;
    zw_bytes* outs = nullptr;
    uint8_t* const* dst = nullptr;
    size_t extra_per_frame() const override { return fbytes; }
    int enqueue(zw_ctx* ctx, DecChunk& C) override
    {
        const DecMeta& M = C.meta;
        for (int i = 0; i < M.n; i++)
            if ((size_t)M.F[i].width != w || (size_t)M.F[i].height != h) return ZW_EINVAL;
        hipStream_t s = ctx_stream(ctx);
        HIPOK(zwk_yuv2rgb(s, C.d + C.lay.y, C.d + C.lay.u, C.d + C.lay.v, M.ysz, M.csz, (int)w, (int)h, M.mbw * 16,
                          M.mbw * 8, bpp, fancy, C.d + C.lay.extra, M.n));
        HIPOK(hipEventRecord(C.set->ev[DEC_EV_CALLER], s));
        return ZW_OK;
    }
    DecEv wait_event() const override { return DEC_EV_CALLER; }
    size_t staging_per_frame(const DecChunk&) const override { return fbytes; }
    int copy_down(zw_ctx* ctx, const DecChunk& C, uint8_t* hout, int a, int b) override
    {
        return ctx_d2h_stream(ctx, hout + (size_t)a * fbytes, C.d + C.lay.extra + (size_t)a * fbytes,
                              (size_t)(b - a) * fbytes);
    }
    bool place(const DecChunk& C, const uint8_t* hout, int i) override
    {
        const uint8_t* src = hout + (size_t)i * fbytes;
        if (dst) {
            uint8_t* o = dst[C.first + i];
            if (stride == row) {
                memcpy(o, src, fbytes);
            } else {
                for (size_t y = 0; y < h; y++) memcpy(o + y * stride, src + y * row, row);
            }
            return true;
        }
        uint8_t* buf = frame_pool().get(fbytes ? fbytes : 1);
        if (!buf) return false;
        memcpy(buf, src, fbytes);
        outs[C.first + i].data = buf;
        outs[C.first + i].len = fbytes;
        return true;
    }
};

// Frame::fill_rgb / fill_rgba (decoder/vp8.rs:200-258) after decode_frame, on
// the device: decode -> k_yuv2rgb -> packed RGB(A) down.  Every frame of the
// batch must have the same dimensions (their packed images are contiguous).
// The images land either in new buffers (outs) or in the caller's buffers
// (dst[i], dst_lens[i] bytes, rows `stride` bytes apart: decode_rgba_into /
// decode_rgb_into, api.rs:1004-1128), where a repeated decode touches no fresh
// pages.
static int dec_rgb_batch(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, int bpp, int upsampling,
                         zw_bytes* outs, uint8_t* const* dst, const size_t* dst_lens, size_t stride, uint32_t* widths,
                         uint32_t* heights)
{
    if (!ctx || n <= 0 || !data || !lens || (!outs && !dst) || (bpp != 3 && bpp != 4) ||
        (upsampling != ZW_UPSAMPLE_BILINEAR && upsampling != ZW_UPSAMPLE_SIMPLE))
        return ZW_EINVAL;
    if (outs)
        for (int i = 0; i < n; i++) outs[i].data = nullptr, outs[i].len = 0;
    RgbSink sink;
    {  // dimensions first (they size the device output)
        DecFrame f0;
        const int r = parse_header(f0, data[0], lens[0]);
        if (r) return r;
        sink.w = f0.width;
        sink.h = f0.height;
    }
    sink.row = sink.w * (size_t)bpp;
    sink.fbytes = sink.row * sink.h;
    if (dst) {  // decode_rgba_into: stride >= width * bpp, buffer >= stride * height
        if (!dst_lens || stride < sink.row) return ZW_EINVAL;
        for (int i = 0; i < n; i++)
            if (!dst[i] || dst_lens[i] < stride * sink.h) return ZW_EINVAL;
    }
    sink.stride = stride;
    sink.bpp = bpp;
    sink.fancy = upsampling == ZW_UPSAMPLE_BILINEAR;
    sink.outs = outs;
    sink.dst = dst;
    const int r = DecRun(ctx, n, data, lens, sink).run();
    if (r) {
        if (outs)
            for (int k = 0; k < n; k++) zw_bytes_free(&outs[k]);
        return r;
    }
    for (int i = 0; i < n; i++) {
        if (widths) widths[i] = (uint32_t)sink.w;
        if (heights) heights[i] = (uint32_t)sink.h;
    }
    return ZW_OK;
}

}  // namespace

extern "C" int zw_vp8_decode_rgb_batch(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, int bpp,
                                       int upsampling, zw_bytes* outs, uint32_t* widths, uint32_t* heights)
{
    if (!outs || n <= 0 || !data || !lens) return ZW_EINVAL;
    for (int i = 0; i < n; i++) outs[i].data = nullptr, outs[i].len = 0;
    int done = 0;  // frames of the runs already decoded
    const int r = for_each_run(n, data, lens, [&](int i0, int i1) {
        done = i0;
        return dec_rgb_batch(ctx, i1 - i0, data + i0, lens + i0, bpp, upsampling, outs + i0, nullptr, nullptr, 0,
                             widths ? widths + i0 : nullptr, heights ? heights + i0 : nullptr);
    });
    if (r)
        for (int k = 0; k < done; k++) zw_bytes_free(&outs[k]);
    return r;
}

extern "C" int zw_vp8_decode_rgb_batch_into(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens,
                                            int bpp, int upsampling, uint8_t* const* outs, const size_t* out_lens,
                                            uint32_t stride_bytes, uint32_t* widths, uint32_t* heights)
{
    if (!outs || n <= 0 || !data || !lens || !out_lens) return ZW_EINVAL;
    return for_each_run(n, data, lens, [&](int i0, int i1) {
        return dec_rgb_batch(ctx, i1 - i0, data + i0, lens + i0, bpp, upsampling, nullptr, outs + i0, out_lens + i0,
                             stride_bytes, widths ? widths + i0 : nullptr, heights ? heights + i0 : nullptr);
    });
}

namespace {

// zw_vp8_decode_batch_device's output: k_yuv2rgb_dev after the filter, from the
// planes straight into the caller's device memory.  Nothing comes down.
struct DeviceSink : DecSink {
    size_t w = 0, h = 0, elsize = 0;
    int layout = 0, dtype = 0, channels = 0, fancy = 0;
    uint8_t* data = nullptr;
    ZwY2rDev P = {};
    size_t extra_per_frame() const override { return 0; }
    // checks the chunk's sizes and queues the colour conversion
    int convert(zw_ctx* ctx, DecChunk& C)
    {
        const DecMeta& M = C.meta;
        for (int i = 0; i < M.n; i++)
            if ((size_t)M.F[i].width != w || (size_t)M.F[i].height != h) return ZW_EINVAL;
        HIPOK(zwk_yuv2rgb_dev(ctx_stream(ctx), C.d + C.lay.y, C.d + C.lay.u, C.d + C.lay.v, M.ysz, M.csz, (int)w, (int)h,
                              M.mbw * 16, M.mbw * 8, layout, dtype, channels, fancy,
                              data + (size_t)C.first * P.frame_stride * elsize, &P, M.n));
        return ZW_OK;
    }
    int enqueue(zw_ctx* ctx, DecChunk& C) override
    {
        if (int r = convert(ctx, C)) return r;
        HIPOK(hipEventRecord(C.set->ev[DEC_EV_CALLER], ctx_stream(ctx)));
        return ZW_OK;
    }
    DecEv wait_event() const override { return DEC_EV_CALLER; }
    size_t staging_per_frame(const DecChunk&) const override { return 0; }
    int copy_down(zw_ctx*, const DecChunk&, uint8_t*, int, int) override { return ZW_OK; }
    bool place(const DecChunk&, const uint8_t*, int) override { return true; }
};

// a + b * c in size_t; false on overflow
static bool madd(size_t a, size_t b, size_t c, size_t* out)
{
    size_t t;
    return !__builtin_mul_overflow(b, c, &t) && !__builtin_add_overflow(a, t, out);
}

// The device entries' checks of a zw_device_images, both made before anything
// is queued.  Its layout, dtype, channels and upsampling:
static bool device_format_ok(const zw_device_images* out)
{
    return (out->layout == ZW_LAYOUT_HWC || out->layout == ZW_LAYOUT_CHW) &&
           (out->dtype == ZW_DTYPE_U8 || out->dtype == ZW_DTYPE_F16 || out->dtype == ZW_DTYPE_F32) &&
           (out->channels == 3 || out->channels == 4) &&
           (out->upsampling == ZW_UPSAMPLE_BILINEAR || out->upsampling == ZW_UPSAMPLE_SIMPLE);
}
// ... and that n frames of w x h fit it: the stride bounds, no overlapping
// frames, capacity >= the last addressed element + 1, `data` aligned to its
// element and device memory on the context's device.  *elsize = the element's bytes.
static int check_device_extent(zw_ctx* ctx, const zw_device_images* out, size_t N, size_t w, size_t h, size_t* elsize)
{
    const size_t ch = (size_t)out->channels;
    // the elements one frame spans, then the last element the batch addresses
    const bool chw = out->layout == ZW_LAYOUT_CHW;
    size_t span = 0, last = 0;
    if (chw) {
        size_t plane = 0;
        if (out->row_stride < w || !madd(w, h - 1, out->row_stride, &plane) || out->plane_stride < plane ||
            !madd(plane, ch - 1, out->plane_stride, &span))
            return ZW_EINVAL;
    } else {
        size_t row = 0;
        if (!madd(0, w, ch, &row) || out->row_stride < row || !madd(row, h - 1, out->row_stride, &span)) return ZW_EINVAL;
    }
    if (N > 1 && out->frame_stride < span) return ZW_EINVAL;  // frames must not overlap
    if (!madd(span, N - 1, out->frame_stride, &last) || out->capacity < last) return ZW_EINVAL;
    *elsize = out->dtype == ZW_DTYPE_U8 ? 1 : (out->dtype == ZW_DTYPE_F16 ? 2 : 4);
    // device memory on the context's device, whole elements
    size_t bytes = 0;
    if (!madd(0, out->capacity, *elsize, &bytes) || ((uintptr_t)out->data & (*elsize - 1))) return ZW_EINVAL;
    HIPOK(hipSetDevice(ctx->device));
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, out->data) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer)
        return ZW_EINVAL;
    }
    if (at.type != hipMemoryTypeDevice || at.device != ctx->device) return ZW_EINVAL;
    return ZW_OK;
}

// The caller's strides, scale and bias as the conversion kernels take them.
static ZwY2rDev device_strides(const zw_device_images* out)
{
    ZwY2rDev P = {};
    P.frame_stride = out->frame_stride;
    P.plane_stride = out->plane_stride;
    P.row_stride = out->row_stride;
    for (int c = 0; c < 4; c++) {
        P.scale[c] = out->scale[c];
        P.bias[c] = out->bias[c];
    }
    return P;
}

}  // namespace

namespace {

// zw_webp_decode_batch_device's output with ZW_WEBP_ALPHA: DeviceSink's colour
// conversion with 4 channels, then the chunk's alpha planes.  A frame's ALPH
// payload (alph[i]; NULL: the file has no alpha flag and keeps 255) is read on
// the host threads (zw_alph_read, one frame per task) into pinned staging,
// started before the chunk's device work is queued so that the two overlap;
// enqueue uploads the chunk's table and planes into its scratch (lay.extra:
// the ZwAlphaFrame entries, the three filters' lists of planes, the planes),
// runs the filter kernels over each filter's planes and k_alpha_store.
struct AlphaDeviceSink : DeviceSink {
    const uint8_t* const* alph = nullptr;
    const size_t* alph_len = nullptr;
    size_t pstride = 0;
    std::thread worker;     // the chunk's ALPH reads
    std::vector<int> rc;    // their codes, per frame of the chunk
    uint8_t* stage = nullptr;
    int staged = 0, nplanes = 0, nlist[4] = {0, 0, 0, 0};
    bool oom = false;
    double host_ms = 0;     // written by the worker, read after its join
    struct Ev {
        hipEvent_t e[3];    // upload queued, filters done, store done
    };
    std::vector<Ev> evs;

    ~AlphaDeviceSink() override
    {
        if (worker.joinable()) worker.join();
        for (Ev& v : evs)
            for (hipEvent_t e : v.e) (void)hipEventDestroy(e);
    }
    static size_t head_bytes(int cnt) { return (size_t)cnt * (sizeof(ZwAlphaFrame) + 16); }
    size_t extra_per_frame() const override { return sizeof(ZwAlphaFrame) + 16 + pstride; }
    void begin_chunk(zw_ctx* ctx, int first, int cnt, int set) override
    {
        if (worker.joinable()) worker.join();
        rc.assign((size_t)cnt, ZW_OK);
        staged = cnt;
        nplanes = nlist[1] = nlist[2] = nlist[3] = 0;
        int na = 0;
        for (int i = 0; i < cnt; i++) na += alph[first + i] != nullptr;
        stage = (uint8_t*)ctx->pin[PIN_ALPHA0 + set].reserve(head_bytes(cnt) + (size_t)na * pstride);
        oom = stage == nullptr;
        if (oom || na == 0) return;
        ZwAlphaFrame* tab = (ZwAlphaFrame*)stage;
        uint32_t* lists = (uint32_t*)(stage + (size_t)cnt * sizeof(ZwAlphaFrame));
        for (int i = 0; i < cnt; i++) {
            const uint8_t* a = alph[first + i];
            if (!a) {
                tab[i] = ZwAlphaFrame{0, 0, 0, 0};
                continue;
            }
            const uint32_t filter = alph_len[first + i] ? (a[0] >> 2) & 3u : 0u;  // (an empty payload fails its read)
            tab[i] = ZwAlphaFrame{1, filter, (uint32_t)nplanes, 0};
            if (filter) lists[(size_t)(filter - 1) * cnt + nlist[filter]++] = (uint32_t)nplanes;
            nplanes++;
        }
        worker = std::thread([this, first, cnt, tab]() {
            const double t0 = dec_now_ms();
            uint8_t* planes = stage + head_bytes(cnt);
            parallel_for(cnt, [&](int i) {
                if (!tab[i].has_alpha) return;
                int filter = 0;
                rc[i] = zw_alph_read(alph[first + i], alph_len[first + i], (uint32_t)w, (uint32_t)h,
                                     planes + (size_t)tab[i].plane * pstride, &filter);
            });
            host_ms += dec_now_ms() - t0;
        });
    }
    int enqueue(zw_ctx* ctx, DecChunk& C) override
    {
        if (worker.joinable()) worker.join();
        const DecMeta& M = C.meta;
        if (oom) return ZW_ENOMEM;
        if (staged != M.n) return ZW_EINVAL;
        for (int i = 0; i < M.n; i++)
            if (rc[i]) return rc[i];
        if (int r = DeviceSink::convert(ctx, C)) return r;
        hipStream_t s = ctx_stream(ctx);
        if (nplanes > 0) {
            uint8_t* dx = C.d + C.lay.extra;
            const size_t head = head_bytes(M.n);
            Ev v;
            for (hipEvent_t& e : v.e) HIPOK(hipEventCreate(&e));
            evs.push_back(v);
            HIPOK(hipMemcpyAsync(dx, stage, head + (size_t)nplanes * pstride, hipMemcpyHostToDevice, s));
            HIPOK(hipEventRecord(v.e[0], s));
            const uint32_t* d_lists = (const uint32_t*)(dx + (size_t)M.n * sizeof(ZwAlphaFrame));
            for (int f = 1; f <= 3; f++)
                HIPOK(zwk_alpha_unfilter(s, dx + head, pstride, (int)w, (int)h, f, d_lists + (size_t)(f - 1) * M.n, nlist[f]));
            HIPOK(hipEventRecord(v.e[1], s));
            HIPOK(zwk_alpha_store(s, dx + head, pstride, (const ZwAlphaFrame*)dx, (int)w, (int)h, layout, dtype,
                                  data + (size_t)C.first * P.frame_stride * elsize, &P, M.n));
            HIPOK(hipEventRecord(v.e[2], s));
        }
        HIPOK(hipEventRecord(C.set->ev[DEC_EV_CALLER], s));
        return ZW_OK;
    }
    // after the run: the call's alpha times into the context
    void collect(zw_ctx* ctx)
    {
        if (worker.joinable()) worker.join();
        ctx->alpha_ms[0] = (float)host_ms;
        for (Ev& v : evs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, v.e[0], v.e[1]) == hipSuccess) ctx->alpha_ms[1] += ms;
            if (hipEventElapsedTime(&ms, v.e[1], v.e[2]) == hipSuccess) ctx->alpha_ms[2] += ms;
        }
    }
};

// zw_vp8_decode_batch_device, and with `alph` (n entries) the alpha form.
static int device_batch(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens, const zw_device_images* out,
                        uint32_t* width, uint32_t* height, const uint8_t* const* alph, const size_t* alph_len)
{
    if (!ctx || n <= 0 || !data || !lens || !out || !out->data) return ZW_EINVAL;
    if (!device_format_ok(out)) return ZW_EINVAL;
    if (alph && out->channels != 4) return ZW_EINVAL;
    for (int i = 0; i < n; i++)
        if (!data[i] && lens[i]) return ZW_EINVAL;
    AlphaDeviceSink asink;
    DeviceSink dsink;
    DeviceSink& sink = alph ? asink : dsink;
    {  // dimensions first (they bound what the kernel addresses)
        DecFrame f0;
        const int r = parse_header(f0, data[0], lens[0]);
        if (r) return r;
        sink.w = f0.width;
        sink.h = f0.height;
    }
    const size_t w = sink.w, h = sink.h;
    if (w == 0 || h == 0) return ZW_EINVALID_DIMENSIONS;
    for (int i = 1; i < n; i++) {  // one size per batch (a frame too short for dimensions reports its own error)
        int wi = 0, hi = 0;
        if (peek_dims(data[i], lens[i], &wi, &hi) && ((size_t)wi != w || (size_t)hi != h)) return ZW_EINVAL;
    }
    if (int r = check_device_extent(ctx, out, (size_t)n, w, h, &sink.elsize)) return r;
    sink.layout = out->layout;
    sink.dtype = out->dtype;
    sink.channels = out->channels;
    sink.fancy = out->upsampling == ZW_UPSAMPLE_BILINEAR;
    sink.data = (uint8_t*)out->data;
    sink.P = device_strides(out);
    if (alph) {
        asink.alph = alph;
        asink.alph_len = alph_len;
        asink.pstride = zw_alpha_plane_stride(w, h);
        ctx->alpha_ms[0] = ctx->alpha_ms[1] = ctx->alpha_ms[2] = 0.f;
    }
    const int r = DecRun(ctx, n, data, lens, sink).run();
    if (alph) asink.collect(ctx);
    if (r) return r;
    if (width) *width = (uint32_t)w;
    if (height) *height = (uint32_t)h;
    return ZW_OK;
}

}  // namespace

extern "C" int zw_vp8_decode_batch_device(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens,
                                          const zw_device_images* out, uint32_t* width, uint32_t* height)
{
    return device_batch(ctx, n, data, lens, out, width, height, nullptr, nullptr);
}

extern "C" int zw_webp_decode_batch_device(zw_ctx* ctx, int n, const uint8_t* const* files, const size_t* lens,
                                           int flags, const zw_device_images* out, uint32_t* width, uint32_t* height)
{
    if (!ctx || n <= 0 || !files || !lens || !out || !out->data || (flags & ~(ZW_WEBP_ALPHA | ZW_WEBP_LOSSLESS)))
        return ZW_EINVAL;
    if (!device_format_ok(out)) return ZW_EINVAL;
    const bool alpha = (flags & ZW_WEBP_ALPHA) != 0;
    if (alpha && out->channels != 4) return ZW_EINVAL;
    std::vector<const uint8_t*> vp8((size_t)n), alph((size_t)n, nullptr);
    std::vector<size_t> vlen((size_t)n), alen((size_t)n, 0);
    std::vector<uint8_t> lossless((size_t)n, 0), ll_alpha((size_t)n, 0);
    std::vector<std::pair<uint32_t, uint32_t>> dims((size_t)n);  // each file's canvas
    uint32_t cw = 0, chh = 0;
    bool any_lossless = false;
    for (int i = 0; i < n; i++) {
        if (!files[i] && lens[i]) return ZW_EINVAL;
        zw_webp_info_ex info;
        if (int r = zw_webp_parse_ex(files[i], lens[i], flags, &info)) return r;
        vp8[i] = files[i] + info.vp8_offset;
        vlen[i] = (size_t)info.vp8_len;
        dims[i] = {info.width, info.height};
        if (i == 0) cw = info.width, chh = info.height;
        if (info.is_lossless) {
            // read_image: the VP8L header against the canvas (decode_frame, decoder/lossless.rs:103-118)
            uint32_t lw = 0, lh = 0;
            if (int r = zwvp8l::read_header(vp8[i], vlen[i], &lw, &lh)) return r;
            if (lw != info.width || lh != info.height) return ZW_EINCONSISTENT_SIZES;
            lossless[i] = 1;
            ll_alpha[i] = info.has_alpha != 0;
            any_lossless = true;
            continue;
        }
        int fw = 0, fh = 0;  // read_image: InconsistentImageSizes (decoder/api.rs:668-670)
        if (peek_dims(vp8[i], vlen[i], &fw, &fh) && ((uint32_t)fw != info.width || (uint32_t)fh != info.height))
            return ZW_EINCONSISTENT_SIZES;
        if (alpha && info.has_alpha) {
            alph[i] = files[i] + info.alph_offset;
            alen[i] = (size_t)info.alph_len;
        }
    }
    if (!any_lossless)
        return device_batch(ctx, n, vp8.data(), vlen.data(), out, width, height, alpha ? alph.data() : nullptr,
                            alpha ? alen.data() : nullptr);
    // A batch with lossless files: one size (the first file's canvas), checked
    // with the whole tensor before anything is queued; then maximal runs of one
    // kind, each a pass of its own at the run's frame offset.
    for (int i = 1; i < n; i++)
        if (dims[i].first != cw || dims[i].second != chh) return ZW_EINVAL;
    if (cw == 0 || chh == 0 || cw > 16384 || chh > 16384) return ZW_EINVALID_DIMENSIONS;
    size_t elsize = 0;
    if (int r = check_device_extent(ctx, out, (size_t)n, cw, chh, &elsize)) return r;
    ctx->ll_ms[0] = ctx->ll_ms[1] = ctx->ll_ms[2] = 0.f;
    for (int a = 0; a < n;) {
        int b = a + 1;
        while (b < n && lossless[b] == lossless[a]) b++;
        zw_device_images sub = *out;
        sub.data = (uint8_t*)out->data + (size_t)a * out->frame_stride * elsize;
        sub.capacity = out->capacity - (size_t)a * out->frame_stride;
        if (lossless[a]) {
            ZwLlOut O;
            O.layout = out->layout;
            O.dtype = out->dtype;
            O.channels = out->channels;
            O.data = (uint8_t*)sub.data;
            O.elsize = elsize;
            O.P = device_strides(out);
            if (int r = zw_ll_decode_run(ctx, b - a, vp8.data() + a, vlen.data() + a, ll_alpha.data() + a, cw, chh, O))
                return r;
        } else {
            uint32_t rw = 0, rh = 0;
            if (int r = device_batch(ctx, b - a, vp8.data() + a, vlen.data() + a, &sub, &rw, &rh,
                                     alpha ? alph.data() + a : nullptr, alpha ? alen.data() + a : nullptr))
                return r;
            if (rw != cw || rh != chh) return ZW_EINVAL;
        }
        a = b;
    }
    if (width) *width = cw;
    if (height) *height = chh;
    return ZW_OK;
}

extern "C" int zw_webp_decode_ex(zw_ctx* ctx, const uint8_t* data, size_t len, int bpp, int upsampling, int flags,
                                 zw_bytes* out, uint32_t* width, uint32_t* height)
{
    if (flags == 0) return zw_webp_decode(ctx, data, len, bpp, upsampling, out, width, height);
    if (!ctx || !out || (flags & ~(ZW_WEBP_ALPHA | ZW_WEBP_LOSSLESS)) || (bpp != 3 && bpp != 4) || (!data && len))
        return ZW_EINVAL;
    if ((flags & ZW_WEBP_ALPHA) && bpp != 4) return ZW_EINVAL;
    out->data = nullptr;
    out->len = 0;
    zw_webp_info_ex info;
    if (int r = zw_webp_parse_ex(data, len, flags, &info)) return r;
    const size_t fbytes = (size_t)info.width * info.height * (size_t)bpp;
    HIPOK(hipSetDevice(ctx->device));
    void* d = ctx->alpha_tmp.reserve(fbytes);
    if (!d) return ZW_ENOMEM;
    zw_device_images img;
    memset(&img, 0, sizeof img);
    img.data = d;
    img.capacity = fbytes;
    img.layout = ZW_LAYOUT_HWC;
    img.dtype = ZW_DTYPE_U8;
    img.channels = bpp;
    img.upsampling = upsampling;
    img.frame_stride = fbytes;
    img.row_stride = (size_t)info.width * (size_t)bpp;
    const uint8_t* f[1] = {data};
    const size_t l[1] = {len};
    uint32_t w = 0, h = 0;
    if (int r = zw_webp_decode_batch_device(ctx, 1, f, l, flags, &img, &w, &h)) return r;
    uint8_t* buf = frame_pool().get(fbytes);
    if (!buf) return ZW_ENOMEM;
    if (hipMemcpy(buf, d, fbytes, hipMemcpyDeviceToHost) != hipSuccess) {
        if (!zw_dec_pool_put(buf)) free(buf);
        return ZW_EDEVICE;
    }
    out->data = buf;
    out->len = fbytes;
    if (width) *width = w;
    if (height) *height = h;
    return ZW_OK;
}

extern "C" int zw_alph_decode(zw_ctx* ctx, const uint8_t* payload, size_t len, uint32_t width, uint32_t height,
                              uint8_t* plane_out)
{
    if (!ctx || !plane_out || (!payload && len) || width == 0 || height == 0 || width > 16384 || height > 16384)
        return ZW_EINVAL;
    const size_t n = (size_t)width * height, pstride = zw_alpha_plane_stride(width, height);
    HIPOK(hipSetDevice(ctx->device));
    uint8_t* hp = (uint8_t*)ctx->pin[PIN_ALPHA0].reserve(256 + pstride);
    if (!hp) return ZW_ENOMEM;
    int filter = 0;
    if (int r = zw_alph_read(payload, len, width, height, hp + 256, &filter)) return r;
    if (filter) {
        uint8_t* d = (uint8_t*)ctx_scratch(ctx, 256 + pstride);
        if (!d) return ZW_ENOMEM;
        memset(hp, 0, 256);  // the list: plane 0
        hipStream_t s = ctx_stream(ctx);
        HIPOK(hipMemcpyAsync(d, hp, 256 + pstride, hipMemcpyHostToDevice, s));
        HIPOK(zwk_alpha_unfilter(s, d + 256, pstride, (int)width, (int)height, filter, (const uint32_t*)d, 1));
        HIPOK(hipMemcpyAsync(hp + 256, d + 256, n, hipMemcpyDeviceToHost, s));
        HIPOK(hipStreamSynchronize(s));
    }
    memcpy(plane_out, hp + 256, n);
    return ZW_OK;
}

extern "C" int zw_decode_alpha_times(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    for (int i = 0; i < 3; i++) ms[i] = ctx->alpha_ms[i];
    return ZW_OK;
}

namespace {

// zw_vp8_decode_batch_device_resized's output for one group of frames of one
// size: k_yuv2rgb_resize after the filter, from the planes into the frames'
// slots of the caller's batch.  tab[i] = the group's frame i (its slot in the
// batch and its window); a chunk's entries are uploaded in stream order into
// the chunk's own scratch (lay.extra), which lives until the chunk has finished.
// filter ZW_RESIZE_TRIANGLE_AA: the weight kernel and k_yuv2rgb_resize_aa
// instead, with each frame's weight tables (aa) in that scratch after the
// chunk's entries.
struct ResizeSink : DecSink {
    size_t w = 0, h = 0;  // the group's frame size
    int out_w = 0, out_h = 0;
    int layout = 0, dtype = 0, channels = 0, fancy = 0, filter = ZW_RESIZE_BILINEAR;
    uint8_t* data = nullptr;
    ZwY2rDev P = {};
    ZwAaTables aa = {};
    std::vector<ZwResizeFrame> tab;
    size_t extra_per_frame() const override
    {
        return sizeof(ZwResizeFrame) + (filter == ZW_RESIZE_TRIANGLE_AA ? (size_t)aa.stride * 4 : 0);
    }
    int enqueue(zw_ctx* ctx, DecChunk& C) override
    {
        const DecMeta& M = C.meta;
        for (int i = 0; i < M.n; i++)  // (the windows were checked against these dimensions)
            if ((size_t)M.F[i].width != w || (size_t)M.F[i].height != h) return ZW_EINVAL;
        hipStream_t s = ctx_stream(ctx);
        ZwResizeFrame* d_tab = (ZwResizeFrame*)(C.d + C.lay.extra);
        HIPOK(hipMemcpyAsync(d_tab, tab.data() + C.first, (size_t)M.n * sizeof(ZwResizeFrame), hipMemcpyHostToDevice, s));
        if (filter == ZW_RESIZE_TRIANGLE_AA) {
            uint32_t* d_aa = (uint32_t*)(d_tab + M.n);  // (32-byte entries: the tables stay 16-byte aligned)
            HIPOK(zwk_yuv2rgb_resize_aa(s, C.d + C.lay.y, C.d + C.lay.u, C.d + C.lay.v, M.ysz, M.csz, (int)w, (int)h,
                                        M.mbw * 16, M.mbw * 8, layout, dtype, channels, fancy, data, &P, d_tab, d_aa,
                                        &aa, out_w, out_h, M.n));
        } else {
            HIPOK(zwk_yuv2rgb_resize(s, C.d + C.lay.y, C.d + C.lay.u, C.d + C.lay.v, M.ysz, M.csz, (int)w, (int)h,
                                     M.mbw * 16, M.mbw * 8, layout, dtype, channels, fancy, data, &P, d_tab, out_w,
                                     out_h, M.n));
        }
        HIPOK(hipEventRecord(C.set->ev[DEC_EV_CALLER], s));
        return ZW_OK;
    }
    DecEv wait_event() const override { return DEC_EV_CALLER; }
    size_t staging_per_frame(const DecChunk&) const override { return 0; }
    int copy_down(zw_ctx*, const DecChunk&, uint8_t*, int, int) override { return ZW_OK; }
    bool place(const DecChunk&, const uint8_t*, int) override { return true; }
};

// The weight tables of one frame of w x h (any window of it) to ow x oh
// (ZwAaTables, zw_common.h): per axis first and count per output index, then
// ceil(2 max(size, out) / out) u16 weights per output index.  false: too large
// for 32-bit word offsets.
static bool aa_tables(size_t w, size_t h, size_t ow, size_t oh, ZwAaTables* L)
{
    const size_t kx = (2 * std::max(w, ow) + ow - 1) / ow, ky = (2 * std::max(h, oh) + oh - 1) / oh;
    size_t o = 0;
    L->xfirst = (uint32_t)o, o += ow;
    L->xcount = (uint32_t)o, o += ow;
    L->yfirst = (uint32_t)o, o += oh;
    L->ycount = (uint32_t)o, o += oh;
    L->xw = (uint32_t)o, o += (kx * ow + 1) / 2;
    L->yw = (uint32_t)o, o += (ky * oh + 1) / 2;
    o = (o + 3) & ~(size_t)3;
    L->stride = (uint32_t)o;
    L->kx = (uint32_t)kx;
    L->ky = (uint32_t)ky;
    return o < ((size_t)1 << 30);
}

}  // namespace

extern "C" int zw_vp8_decode_batch_device_resized_ex(zw_ctx* ctx, int n, const uint8_t* const* data,
                                                     const size_t* lens, const zw_device_images* out, uint32_t out_w,
                                                     uint32_t out_h, const zw_rect* windows, uint32_t* widths,
                                                     uint32_t* heights, int filter)
{
    if (!ctx || n <= 0 || !data || !lens || !out || !out->data) return ZW_EINVAL;
    if (filter != ZW_RESIZE_BILINEAR && filter != ZW_RESIZE_TRIANGLE_AA) return ZW_EINVAL;
    if (out_w == 0 || out_h == 0 || out_w > (1u << 20) || out_h > (1u << 20)) return ZW_EINVAL;
    if (!device_format_ok(out)) return ZW_EINVAL;
    for (int i = 0; i < n; i++)
        if (!data[i] && lens[i]) return ZW_EINVAL;
    size_t elsize = 0;
    if (int r = check_device_extent(ctx, out, (size_t)n, out_w, out_h, &elsize)) return r;
    // The frames' sizes and windows, and the groups: the indices of each size
    // in frame order, the sizes in order of first appearance.  A frame whose
    // header gives no usable size stands alone; its decode reports its error.
    const uint32_t NO_DIMS = 0xffffffffu;
    std::vector<uint32_t> key(n);
    std::vector<ZwResizeFrame> win(n);
    for (int i = 0; i < n; i++) {
        int w = 0, h = 0;
        const bool dims = peek_dims(data[i], lens[i], &w, &h) && w > 0 && h > 0;
        key[i] = dims ? (uint32_t)w | ((uint32_t)h << 16) : NO_DIMS;
        const zw_rect r = windows ? windows[i] : zw_rect{0, 0, (uint32_t)w, (uint32_t)h};
        if (windows && (r.w == 0 || r.h == 0)) return ZW_EINVAL;
        if (dims && ((uint64_t)r.x + r.w > (uint64_t)w || (uint64_t)r.y + r.h > (uint64_t)h)) return ZW_EINVAL;
        win[i] = ZwResizeFrame{(uint32_t)i, r.x, r.y, r.w, r.h, {0, 0, 0}};
        ZwAaTables t;  // (a frame's weight tables must fit 32-bit offsets: also before anything is queued)
        if (filter == ZW_RESIZE_TRIANGLE_AA && !aa_tables((size_t)w, (size_t)h, out_w, out_h, &t)) return ZW_ENOMEM;
    }
    std::vector<std::vector<int>> groups;
    {
        std::unordered_map<uint32_t, size_t> at;
        for (int i = 0; i < n; i++) {
            auto it = key[i] == NO_DIMS ? at.end() : at.find(key[i]);
            if (it == at.end()) {
                if (key[i] != NO_DIMS) at[key[i]] = groups.size();
                groups.emplace_back(1, i);
            } else {
                groups[it->second].push_back(i);
            }
        }
    }
    // One decode pass (DecRun) per group; the batch's times are the groups' sums.
    float dec_ms[3] = {0.f, 0.f, 0.f}, tok_ms = 0.f, tok_stage_ms[3] = {0.f, 0.f, 0.f};
    double host_ms[3] = {0, 0, 0};
    int err = ZW_OK;
    for (size_t g = 0; g < groups.size() && !err; g++) {
        const std::vector<int>& idx = groups[g];
        const uint32_t k = key[idx[0]];
        ResizeSink sink;
        sink.w = k == NO_DIMS ? 0 : (k & 0xffffu);
        sink.h = k == NO_DIMS ? 0 : (k >> 16);
        sink.out_w = (int)out_w;
        sink.out_h = (int)out_h;
        sink.layout = out->layout;
        sink.dtype = out->dtype;
        sink.channels = out->channels;
        sink.fancy = out->upsampling == ZW_UPSAMPLE_BILINEAR;
        sink.data = (uint8_t*)out->data;
        sink.P = device_strides(out);
        sink.filter = filter;
        if (filter == ZW_RESIZE_TRIANGLE_AA) (void)aa_tables(sink.w, sink.h, out_w, out_h, &sink.aa);  // (checked above)
        std::vector<const uint8_t*> gdata(idx.size());
        std::vector<size_t> glens(idx.size());
        sink.tab.resize(idx.size());
        for (size_t j = 0; j < idx.size(); j++) {
            gdata[j] = data[idx[j]];
            glens[j] = lens[idx[j]];
            sink.tab[j] = win[idx[j]];
        }
        err = DecRun(ctx, (int)idx.size(), gdata.data(), glens.data(), sink).run();
        for (int t = 0; t < 3; t++) {
            dec_ms[t] += ctx->dec_ms[t];
            tok_stage_ms[t] += ctx->dec_tok_stage_ms[t];
            host_ms[t] += ctx->dec_host_ms[t];
        }
        tok_ms += ctx->dec_tok_ms;
    }
    for (int t = 0; t < 3; t++) {
        ctx->dec_ms[t] = dec_ms[t];
        ctx->dec_tok_stage_ms[t] = tok_stage_ms[t];
        ctx->dec_host_ms[t] = host_ms[t];
    }
    ctx->dec_tok_ms = tok_ms;
    if (err) return err;
    for (int i = 0; i < n; i++) {
        if (widths) widths[i] = key[i] & 0xffffu;
        if (heights) heights[i] = key[i] >> 16;
    }
    return ZW_OK;
}

extern "C" int zw_vp8_decode_batch_device_resized(zw_ctx* ctx, int n, const uint8_t* const* data, const size_t* lens,
                                                  const zw_device_images* out, uint32_t out_w, uint32_t out_h,
                                                  const zw_rect* windows, uint32_t* widths, uint32_t* heights)
{
    return zw_vp8_decode_batch_device_resized_ex(ctx, n, data, lens, out, out_w, out_h, windows, widths, heights,
                                                 ZW_RESIZE_BILINEAR);
}

extern "C" int zw_vp8_decode_rgb(zw_ctx* ctx, const uint8_t* vp8, size_t len, int bpp, int upsampling, zw_bytes* out,
                                 uint32_t* width, uint32_t* height)
{
    if (!vp8 && len) return ZW_EINVAL;
    const uint8_t* d[1] = {vp8};
    size_t l[1] = {len};
    return zw_vp8_decode_rgb_batch(ctx, 1, d, l, bpp, upsampling, out, width, height);
}

// Kernel-level entry: fill_rgb_buffer_fancy / _simple (decoder/yuv.rs:82, :402)
// of one image's planes (host buffers; rows of y_stride / uv_stride bytes,
// ceil(h/2) chroma rows) into out (w*h*bpp bytes, packed).
extern "C" int zw_yuv_to_rgb(zw_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t width,
                             uint32_t height, uint32_t y_stride, uint32_t uv_stride, int bpp, int upsampling,
                             uint8_t* out)
{
    if (!ctx || !y || !u || !v || !out || width == 0 || height == 0 || y_stride < width ||
        uv_stride < (width + 1) / 2 || (bpp != 3 && bpp != 4) ||
        (upsampling != ZW_UPSAMPLE_BILINEAR && upsampling != ZW_UPSAMPLE_SIMPLE))
        return ZW_EINVAL;
    const size_t ch = (height + 1) / 2;
    const size_t ysz = (size_t)y_stride * height, csz = (size_t)uv_stride * ch;
    const size_t obytes = (size_t)width * height * bpp;
    const size_t o_y = 0, o_u = al256(ysz), o_v = al256(o_u + csz), o_o = al256(o_v + csz);
    HIPOK(hipSetDevice(ctx->device));
    uint8_t* d = (uint8_t*)ctx_scratch(ctx, al256(o_o + obytes));
    if (!d) return ZW_ENOMEM;
    hipStream_t s = ctx_stream(ctx);
    HIPOK(hipMemcpyAsync(d + o_y, y, ysz, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + o_u, u, csz, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + o_v, v, csz, hipMemcpyHostToDevice, s));
    HIPOK(zwk_yuv2rgb(s, d + o_y, d + o_u, d + o_v, ysz, csz, (int)width, (int)height, (int)y_stride, (int)uv_stride,
                      bpp, upsampling == ZW_UPSAMPLE_BILINEAR, d + o_o, 1));
    HIPOK(hipMemcpyAsync(out, d + o_o, obytes, hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    return ZW_OK;
}

extern "C" int zw_decode_kernel_times(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    ms[0] = ctx->dec_ms[0];
    ms[1] = ctx->dec_ms[1];
    return ZW_OK;
}

extern "C" int zw_decode_token_ms(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    *ms = ctx->dec_tok_ms;
    return ZW_OK;
}

extern "C" int zw_decode_token_stages(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    for (int i = 0; i < 3; i++) ms[i] = ctx->dec_tok_stage_ms[i];
    return ZW_OK;
}

extern "C" int zw_decode_stage_times(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    for (int i = 0; i < 3; i++) ms[i] = (float)ctx->dec_host_ms[i];
    return ZW_OK;
}

extern "C" int zw_decode_rgb_kernel_ms(zw_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return ZW_EINVAL;
    *ms = ctx->dec_ms[2];
    return ZW_OK;
}

extern "C" int zw_vp8_decode_frame(zw_ctx* ctx, const uint8_t* vp8, size_t len, zw_frame* out)
{
    if (!vp8 && len) return ZW_EINVAL;
    const uint8_t* d[1] = {vp8};
    size_t l[1] = {len};
    return zw_vp8_decode_batch(ctx, 1, d, l, out);
}

extern "C" int zw_loop_filter_frame(zw_ctx* ctx, uint8_t* y, uint8_t* u, uint8_t* v, uint32_t mbw, uint32_t mbh,
                                    const uint8_t* mb_flags, int filter_type, int filter_level, int sharpness,
                                    int segments_enabled, int seg_delta_values, const int8_t seg_lf_level[4],
                                    int lf_adj_enabled, int ref_delta0, int mode_delta0)
{
    if (!ctx || !y || !u || !v || !mb_flags || mbw == 0 || mbh == 0) return ZW_EINVAL;
    const int8_t zero[4] = {0, 0, 0, 0};
    ZwFilterParams fp;
    filter_table(fp, filter_type, filter_level, sharpness, segments_enabled, seg_delta_values,
                 seg_lf_level ? seg_lf_level : zero, lf_adj_enabled, ref_delta0, mode_delta0, (int)mbw, (int)mbh);
    const size_t nmb = (size_t)mbw * mbh, ysz = nmb * 256, csz = nmb * 64;
    const DecKnobs K;
    const bool rows = K.rows != 0;  // (one frame: the row-parallel filter unless ZW_DEC_ROWS=0)
    // one frame of the batch layout with nothing uploaded: the filter table, the flags, the planes, the sync words
    const DecLayout L = dec_layout(1, (int)mbw, (int)mbh, rows, 0, 0);
    HIPOK(hipSetDevice(ctx->device));
    uint8_t* d = (uint8_t*)ctx_scratch(ctx, L.total);
    if (!d) return ZW_ENOMEM;
    hipStream_t s = ctx_stream(ctx);
    const ZwFilterParams* d_fp = (const ZwFilterParams*)(d + L.fparams);
    int* d_rs = (int*)(d + L.rowsync);
    HIPOK(hipMemcpyAsync(d + L.fparams, &fp, sizeof fp, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.flags, mb_flags, nmb * 4, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.y, y, ysz, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.u, u, csz, hipMemcpyHostToDevice, s));
    HIPOK(hipMemcpyAsync(d + L.v, v, csz, hipMemcpyHostToDevice, s));
    if (rows) {
        HIPOK(zwk_dec_rows_init(s, d_rs, (int)mbh, 1));
        if (K.force_error) HIPOK(hipMemsetAsync(d_rs + 2, 1, sizeof(int), s));
        HIPOK(zwk_dec_rows(s, 2, nullptr, nullptr, nullptr, nullptr, d + L.y, d + L.u, d + L.v, d + L.flags, d_fp,
                           (int)mbw, (int)mbh, ysz, csz, 1, d_rs, nullptr, (int)mbh));
    } else {
        HIPOK(zwk_loopfilter(s, d + L.y, d + L.u, d + L.v, d + L.flags, d_fp, ysz, csz, 1, (int)mbw, nullptr));
    }
    HIPOK(hipMemcpyAsync(y, d + L.y, ysz, hipMemcpyDeviceToHost, s));
    HIPOK(hipMemcpyAsync(u, d + L.u, csz, hipMemcpyDeviceToHost, s));
    HIPOK(hipMemcpyAsync(v, d + L.v, csz, hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    return rows ? rows_error(ctx, d_rs, 1, (int)mbh) : ZW_OK;
}


// decode_rgba_into / decode_rgb_into (decoder/api.rs:1004-1128): a lossy WebP
// file into the caller's buffer with a row stride.
extern "C" int zw_webp_decode_into(zw_ctx* ctx, const uint8_t* data, size_t len, int bpp, int upsampling, uint8_t* out,
                                   size_t out_len, uint32_t stride_bytes, uint32_t* width, uint32_t* height)
{
    if (!ctx || !out) return ZW_EINVAL;
    zw_webp_info info;
    if (int r = zw_webp_parse(data, len, &info)) return r;
    if ((size_t)stride_bytes < (size_t)info.width * bpp || out_len < (size_t)stride_bytes * info.height)
        return ZW_EINVAL;  // InvalidParameter: stride / output buffer too small
    const uint8_t* d[1] = {data + info.vp8_offset};
    const size_t l[1] = {(size_t)info.vp8_len};
    uint8_t* o[1] = {out};
    const size_t ol[1] = {out_len};
    uint32_t w = 0, h = 0;
    if (int r = dec_rgb_batch(ctx, 1, d, l, bpp, upsampling, nullptr, o, ol, stride_bytes, &w, &h)) return r;
    if (w != info.width || h != info.height) return ZW_EINCONSISTENT_SIZES;
    if (width) *width = w;
    if (height) *height = h;
    return ZW_OK;
}

extern "C" int zw_webp_decode(zw_ctx* ctx, const uint8_t* data, size_t len, int bpp, int upsampling, zw_bytes* out,
                              uint32_t* width, uint32_t* height)
{
    if (!ctx || !out) return ZW_EINVAL;
    out->data = nullptr;
    out->len = 0;
    zw_webp_info info;
    if (int r = zw_webp_parse(data, len, &info)) return r;
    uint32_t w = 0, h = 0;
    if (int r = zw_vp8_decode_rgb(ctx, data + info.vp8_offset, (size_t)info.vp8_len, bpp, upsampling, out, &w, &h))
        return r;
    if (w != info.width || h != info.height) {  // read_image: InconsistentImageSizes
        zw_bytes_free(out);
        return ZW_EINCONSISTENT_SIZES;
    }
    if (width) *width = w;
    if (height) *height = h;
    return ZW_OK;
}
