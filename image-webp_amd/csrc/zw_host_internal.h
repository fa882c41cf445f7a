// zw_host_internal.h -- state shared by the host translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

// Set (process-wide) once an SDMA copy timed out with the engine possibly
// still writing its destination: from then on pinned host buffers, which are
// the destinations of those copies, are leaked instead of freed, so a late
// DMA write cannot land in memory the allocator has handed out again.
extern std::atomic<bool> g_dma_poisoned;
static inline void pinned_free(void* h)
{
    if (h && !g_dma_poisoned.load(std::memory_order_acquire)) (void)hipHostFree(h);
}

// A grow-only buffer a context keeps between calls: device memory (DevBuf) or
// pinned host staging (PinBuf, freed by the poisoned-DMA rule above).
template <bool PINNED>
struct __attribute__((visibility("hidden"))) GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    // At least `bytes` (the contents are lost when it grows); nullptr: out of memory.
    void* reserve(size_t bytes)
    {
        if (cap < bytes) {
            release();
            const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
            if (e != hipSuccess) {
                p = nullptr;
                return nullptr;
            }
            cap = bytes;
        }
        return p;
    }
    void release()
    {
        if (PINNED) pinned_free(p);
        else if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};
using DevBuf = GrowBuf<false>;
using PinBuf = GrowBuf<true>;

// The events of one decode buffer set, in stream order.
enum DecEv { DEC_EV_RECON_START, DEC_EV_RECON_DONE, DEC_EV_FILTER_DONE, DEC_EV_CALLER, DEC_EV_COUNT };
// The device token parse's events on its own stream, in the order they are
// recorded: the upload queued, stage 1 done, the count pass and scans done, the
// records written.
enum TokEv { TOK_EV_START, TOK_EV_STAGE1, TOK_EV_COUNTED, TOK_EV_RECORDS, TOK_EV_COUNT };
// Pinned staging shared by both decode buffer sets (each set has its own upload slot).
enum DecPin {
    PIN_DOWNLOAD,    // planes / packed images down
    PIN_ERR_WORDS,   // the row-parallel kernels' sync / error words, the token parse's error words
    PIN_TOK_UPLOAD,  // the device token parse's upload (modes, probabilities, token partitions)
    PIN_ALPHA0,      // the alpha decode's table and planes of a chunk, one per buffer set
    PIN_ALPHA1,
    PIN_VP8L0,       // the lossless decode's table, coded images and transform data of a chunk, one per staging set
    PIN_VP8L1,
    PIN_COUNT
};

struct zw_ctx {
    int device;
    hipStream_t stream_ = nullptr;  // created on first use (hardware queues are scarce)
    hipStream_t copy_ = nullptr;    // decode downloads (ctx_d2h_stream), created on first use
    hipEvent_t copy_ev = nullptr;   // its completion, waited on without spinning
    // decode: per-frame worst-case record buffers, kept between chunks and calls
    // (a parse touches only the pages it writes; reallocating them per chunk
    // cost page faults and unmaps)
    struct RecBuf {
        std::unique_ptr<uint8_t[]> p;  // uninitialised: untouched pages stay unbacked
        size_t cap = 0;
    };
    // One of the two buffer sets the pipelined decode batches alternate between.
    // set[0].scratch is also the device scratch of the single-call decode /
    // filter / transform entry points (ctx_scratch).
    struct __attribute__((visibility("hidden"))) DecSet {
        DevBuf scratch;  // records, tables, planes, the caller's extra (DecLayout)
        PinBuf upload;   // the host parser's records, MB offsets and frame bases
        hipEvent_t ev[DEC_EV_COUNT] = {};  // created on first use (blocking sync: the finisher sleeps on them)
        std::vector<RecBuf> recs;
    };
    DecSet set[2];
    PinBuf pin[PIN_COUNT];
    DevBuf alpha_tmp;    // zw_webp_decode_ex: the RGBA image on the device before its download
    // the alpha work of the last alpha decode: [0] the ALPH payloads on the host
    // threads (wall ms), [1] the filter kernels, [2] k_alpha_store (device ms)
    float alpha_ms[3] = {0.f, 0.f, 0.f};
    // the last lossless decode: [0] the VP8L entropy decode on the host threads
    // (wall ms), [1] the transform kernels, [2] the store kernel (device ms)
    float ll_ms[3] = {0.f, 0.f, 0.f};
    DevBuf tok_scratch;  // the device token parse's upload, snapshots and offsets
    DevBuf tok_recs;     // the device token parse's records (sized by its count pass)
    uint64_t* tok_total = nullptr;  // pinned: the count pass's record bytes
    hipStream_t tok_ = nullptr;  // the device token parse (runs beside the chunks' kernels), created on first use
    hipEvent_t tok_ev[TOK_EV_COUNT] = {};
    // zw_transform_quant_mbs*_device: the I4 queue of k_xform_mb / k_xform_mb_i4,
    // one per launch stream (launches on different streams may overlap; launches
    // on one stream are ordered), its counters reset on that stream per launch
    struct XmbQueue {
        hipStream_t stream = nullptr;
        void* buf = nullptr;
        size_t cap = 0;
        bool dirty = true;  // counters not known to be zero: reset on the stream first
        int parity = 0;     // the count the next launch appends to (k_xform_mb's qp)
        uint64_t used = 0;  // xmb_clock at the last launch (LRU eviction past 8 streams)
        int inflight = 0;   // launches being queued on it (between the two locked sections): not evictable
    };
    std::deque<XmbQueue> xmb_q;  // (a deque: entries stay put while others are added)
    uint64_t xmb_clock = 0;
    volatile uint32_t* xmb_err = nullptr;  // host-mapped: k_xform_mb sets it on a queue overflow
    uint32_t* xmb_err_dev = nullptr;       // the same word as the device addresses it
    std::mutex xmb_mu;
    // SDMA copy engine path (HSA) for device->host fetches: ROCclr's hipMemcpy
    // D2H runs as a blit kernel, which cannot be dispatched while an encode
    // kernel holds every CU; the DMA engines need no CU.
    // Probed once under sdma_mu (pipe lanes call ctx_d2h from several threads).
    std::atomic<int> sdma{-1};  // -1 unprobed, 0 unavailable, 1 ready
    std::mutex sdma_mu;
    // set when a DMA copy did not complete in time: the engine may still write
    // into its destination, so every later copy of this context fails
    std::atomic<bool> poisoned{false};
    hsa_agent_t gpu_agent{}, cpu_agent{};
    // device time of the last decode batch: [0] k_dec_recon, [1] k_loopfilter,
    // [2] k_yuv2rgb (0 when the batch returned planes) (ms)
    float dec_ms[3] = {0.f, 0.f, 0.f};
    float dec_tok_ms = 0.f;  // the device token parse of the last batch (0: the host parsed every frame)
    float dec_tok_stage_ms[3] = {0.f, 0.f, 0.f};  // its stage 1, count pass + offsets (+ the host's wait), record pass
    // measured rates for the host / device split of the token parse (dec_tok_split),
    // both per MB of a frame so that they carry over to a batch of another frame size
    // (a mixed-size batch decodes one size after another): host chunk parse ms per
    // frame (the whole chunk over all threads), device launch ms (the launch runs
    // its frames side by side), 0 = not measured yet
    double dec_host_ms_per_mb = 0, dec_tok_ms_per_mb = 0;
    // host stages of the last decode batch, wall ms summed over its chunks:
    // [0] parse (bool decoder + records), [1] download, [2] fan-out / copy-out
    double dec_host_ms[3] = {0, 0, 0};
    // one-frame encode pipeline kept between encode_frame_lossy calls of the
    // same shape (dimensions, colour type, quality, method): its device buffers
    // and streams are reused instead of allocated per call
    // A call takes the cached pipe out under pipe1_mu and puts it back when it
    // succeeds, so two threads sharing a context never run on one pipe.
    struct zw_pipe* pipe1 = nullptr;
    int pipe1_key[5] = {0, 0, 0, 0, 0};
    std::mutex pipe1_mu;
};

#define HIPOK(x)                                  \
    do {                                          \
        hipError_t e_ = (x);                      \
        if (e_ != hipSuccess) {                   \
            fprintf(stderr, "zwebp: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return ZW_EDEVICE;                    \
        }                                         \
    } while (0)


// Host worker threads per process (entropy coding, stats, decode parsing).
// ZW_HOST_THREADS overrides.  Default: this process's share of the CPUs it may
// run on -- the affinity mask divided by the ranks on this node
// (LOCAL_WORLD_SIZE, set by torch.distributed.run), capped by the job's
// per-process CPU share when one is declared (OMP_NUM_THREADS).
static inline int host_threads_default()
{
    cpu_set_t set;
    int cpus = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 0;
    if (cpus <= 0) cpus = (int)std::thread::hardware_concurrency();
    const char* lw = getenv("LOCAL_WORLD_SIZE");
    const int ranks = lw && atoi(lw) > 0 ? atoi(lw) : 1;
    int n = cpus / ranks;
    const char* omp = getenv("OMP_NUM_THREADS");
    if (omp && atoi(omp) > 0 && atoi(omp) < n) n = atoi(omp);
    return n < 1 ? 1 : n;
}
static inline int host_threads()
{
    const char* e = getenv("ZW_HOST_THREADS");
    int n = e ? atoi(e) : 0;
    if (n <= 0) {
        static const int dflt = host_threads_default();
        n = dflt;
    }
    return n;
}

template <class F>
static inline void parallel_for(int n, F fn, int max_threads = 0)
{
    int nt = std::min(max_threads > 0 ? std::min(max_threads, host_threads()) : host_threads(), n);
    if (nt <= 1) {
        for (int i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<int> next(0);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&]() {
            for (;;) {
                int i = next.fetch_add(1);
                if (i >= n) break;
                fn(i);
            }
        });
    for (auto& t : th) t.join();
}


// Device scratch of at least `bytes` for the single-call entry points.
static inline void* ctx_scratch(zw_ctx* c, size_t bytes) { return c->set[0].scratch.reserve(bytes); }

// The context's own stream (single-call entry points); created lazily so a
// context that only drives pipes does not hold a hardware queue.
// Device->host copy on the context's copy stream (HIP chooses the engine: a
// blit kernel for large copies, ≈57 GB/s on this box against ≈25 GB/s for one
// SDMA engine).  For the decode paths, whose kernels leave CUs free; the encode
// pipeline's fetches keep ctx_d2h (its kernels hold every CU).
int ctx_d2h_stream(zw_ctx* c, void* dst, const void* src, size_t bytes);

static inline hipStream_t ctx_stream(zw_ctx* c)
{
    if (!c->stream_) (void)hipStreamCreateWithFlags(&c->stream_, hipStreamNonBlocking);
    return c->stream_;
}

// Blocking device->host copy on a DMA engine (falls back to hipMemcpy when the
// HSA agents cannot be resolved).  `src` must have been released by the
// producing kernel (event-complete) before the call, and `dst` must be pinned
// (hipHostMalloc): the DMA engine cannot reach pageable memory.
int ctx_d2h(zw_ctx* c, void* dst, const void* src, size_t bytes);

// Decoded-frame buffer pool (zw_dec_host.cpp): takes back a buffer it handed
// out (returns false for any other pointer, which the caller frees).
bool zw_dec_pool_put(void* p);
// Frees the buffers the pool holds (zw_ctx_release_buffers).
void zw_dec_pool_trim();
// Is some zw_ctx alive (zw_host.cpp)?  The frame pool keeps buffers only then.
bool zw_ctx_any_alive();
// Frees a context's resources and the context (zw_ctx_destroy minus the count).
void zw_ctx_free_internal(zw_ctx* c);

// Host lossless coder and container writer (zw_host_lossless.cpp).
int zw_vp8l_encode(const uint8_t* data, size_t len, uint32_t width, uint32_t height, int color, bool predictor,
                   bool implicit_dims, std::vector<uint8_t>& out);
int zw_alph_encode(const uint8_t* data, size_t len, uint32_t width, uint32_t height, int color,
                   std::vector<uint8_t>& out);
void zw_webp_wrap(std::vector<uint8_t>& o, const uint8_t* frame, size_t flen, const char* tag,
                  const std::vector<uint8_t>* alph, bool has_alpha, uint32_t width, uint32_t height,
                  const zw_metadata& md);
