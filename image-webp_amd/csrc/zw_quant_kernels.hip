// zw_quant_kernels.hip -- the block quantisers as kernels of their own (gfx950):
// k_quant_blocks / k_quant_blocks_g run zw_dev.h's quantz, trellis and trellis_g
// over independent blocks (zw_quant_blocks).
#include "zw_dev.h"

// ---------------------------------------------------------------------------
// Kernel-level entry: quantisation (simple or trellis) of independent 4x4
// coefficient blocks, one block per thread (quantize_coeff cost.rs:457,
// trellis_quantize_block cost.rs:788).  Used by the parity tests and as the
// building block the encoder kernels share.
// ---------------------------------------------------------------------------
struct QuantBlocksArgs {
    ZwMatrix m;
    uint16_t sharpen[16];
    uint32_t lambda;
    int32_t ctype, first, trel, n;
};

extern "C" __global__ __launch_bounds__(256) void k_quant_blocks(const int* __restrict__ coeffs,
                                                                const uint8_t* __restrict__ ctx0s,
                                                                const ZwLevelCosts* __restrict__ lcost,
                                                                const uint8_t* __restrict__ probs, QuantBlocksArgs a,
                                                                int* __restrict__ levels, int* __restrict__ dq)
{
    __shared__ LdsTables T;
    for (int i = threadIdx.x; i < (int)(sizeof(T.lc) / 2); i += 256) (&T.lc[0][0][0][0])[i] = (&lcost->lc[0][0][0][0])[i];
    for (int i = threadIdx.x; i < 96; i += 256) {
        (&T.eob[0][0][0])[i] = (&lcost->eob[0][0][0])[i];
        (&T.init[0][0][0])[i] = (&lcost->init[0][0][0])[i];
    }
    for (int i = threadIdx.x; i < 4 * 8 * 3 * 11; i += 256) (&T.probs[0][0][0][0])[i] = probs[i];
    load_static_tables(&T, threadIdx.x, 256, probs);
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.n) return;
    int c[16], lv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) c[k] = coeffs[(size_t)b * 16 + k];
    const int ctx0 = ctx0s[b];
    if (a.trel) {
        if (a.first) trellis<1>(c, lv, a.m, a.sharpen, a.lambda, &T, a.ctype, ctx0);
        else trellis<0>(c, lv, a.m, a.sharpen, a.lambda, &T, a.ctype, ctx0);
        if (a.first) lv[0] = 0;
    } else {
#pragma unroll
        for (int n = 0; n < 16; n++) {
            const int j = kZZ(n);
            lv[n] = n < a.first ? 0 : quantz(c[j], a.m.iq[j > 0], a.m.bias[j > 0]);
        }
#pragma unroll
        for (int n = 0; n < 16; n++) {
            const int j = kZZ(n);
            c[j] = n < a.first ? 0 : m24(lv[n], (int)a.m.q[j > 0]);
        }
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        levels[(size_t)b * 16 + k] = lv[k];
        dq[(size_t)b * 16 + k] = c[k];
    }
}

// The lane-parallel trellis (trellis_g, used by the final I4 pass): 16 lanes
// per block, lane = zigzag position.
extern "C" __global__ __launch_bounds__(256) void k_quant_blocks_g(const int* __restrict__ coeffs,
                                                                  const uint8_t* __restrict__ ctx0s,
                                                                  const ZwLevelCosts* __restrict__ lcost,
                                                                  const uint8_t* __restrict__ probs, QuantBlocksArgs a,
                                                                  int* __restrict__ levels, int* __restrict__ dq)
{
    __shared__ LdsTables T;
    for (int i = threadIdx.x; i < (int)(sizeof(T.lc) / 2); i += 256) (&T.lc[0][0][0][0])[i] = (&lcost->lc[0][0][0][0])[i];
    for (int i = threadIdx.x; i < 96; i += 256) {
        (&T.eob[0][0][0])[i] = (&lcost->eob[0][0][0])[i];
        (&T.init[0][0][0])[i] = (&lcost->init[0][0][0])[i];
    }
    for (int i = threadIdx.x; i < 4 * 8 * 3 * 11; i += 256) (&T.probs[0][0][0][0])[i] = probs[i];
    load_static_tables(&T, threadIdx.x, 256, probs);
    __syncthreads();
    const int b = (int)((blockIdx.x * 256 + threadIdx.x) >> 4), n = threadIdx.x & 15;
    const int bb = min(b, a.n - 1);  // whole groups stay active (DPP/ballot need every lane)
    const int cn = coeffs[(size_t)bb * 16 + zz_of(n)];
    const int ctx0 = ctx0s[bb];
    int lvl;
    if (a.first) (void)trellis_g<1>(cn, n, a.m, a.sharpen, a.lambda, &T, a.ctype, ctx0, lvl);
    else (void)trellis_g<0>(cn, n, a.m, a.sharpen, a.lambda, &T, a.ctype, ctx0, lvl);
    if (b < a.n) {
        const int j = zz_of(n);
        levels[(size_t)b * 16 + n] = lvl;
        // positions before `first` keep their input coefficient (as trellis<1> leaves coeffs[0])
        dq[(size_t)b * 16 + j] = n < a.first ? cn : lvl * (int)(j == 0 ? a.m.q[0] : a.m.q[1]);
    }
}

extern "C" hipError_t zwk_quant_blocks(hipStream_t s, const int* coeffs, const uint8_t* ctx0s, const ZwLevelCosts* lcost,
                                       const uint8_t* probs, const void* args, int* levels, int* dq)
{
    const QuantBlocksArgs& a = *(const QuantBlocksArgs*)args;
    if (a.trel == 2)
        hipLaunchKernelGGL(k_quant_blocks_g, dim3((a.n * 16 + 255) / 256), dim3(256), 0, s, coeffs, ctx0s, lcost, probs,
                           a, levels, dq);
    else
        hipLaunchKernelGGL(k_quant_blocks, dim3((a.n + 255) / 256), dim3(256), 0, s, coeffs, ctx0s, lcost, probs, a,
                           levels, dq);
    return hipGetLastError();
}
