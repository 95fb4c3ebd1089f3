// The glue around GMFlow that FRESCO's FlowCalc.get_flow (src/ebsynth/flow/flow_utils.py) runs per frame pair, batched
// over P pairs of n distinct frames; DESIGN.md section 9.2.
//   input : uint8 HWC frames (BGR, as cv2.imread gives them) -> InputPadder(mode='sintel', padding_factor=8)'s replicate
//           padding -> GMFlow.forward's (x / 255.0 - mean) / std, as torch evaluates it on the device: the division by
//           the Python scalar is a multiplication by its fp32 reciprocal, the other two are tensor ops; not contracted.
//   output: InputPadder.unpad of the network's (2P, 2, H', W') flows, then forward_backward_consistency_check(fwd, bwd)
//           with the unpadded fields (flow_consistency.h, shared with fresco_flow_occlusion).
// One thread per pixel, the batch index in blockIdx.z.
#include "common.h"
#include "flow_consistency.h"

namespace fresco {
namespace {

constexpr int kFcBlock = 16;
constexpr int kFcMaxBatch = 65535;  // grid z

// torch.tensor([0.485, 0.456, 0.406]) / [0.229, 0.224, 0.225] as fp32 (the doubles rounded once)
__constant__ float kMean[3] = {0x1.f0a3d8p-2f, 0x1.d2f1aap-2f, 0x1.9fbe76p-2f};
__constant__ float kStd[3] = {0x1.d4fdf4p-3f, 0x1.cac084p-3f, 0x1.ccccccp-3f};

struct Pads {
    int top, bottom, left, right, hp, wp;
};

// InputPadder(dims, mode='sintel', padding_factor=8)
Pads sintel_pads(int h, int w) {
    const int ph = ((h / 8 + 1) * 8 - h) % 8, pw = ((w / 8 + 1) * 8 - w) % 8;
    return Pads{ph / 2, ph - ph / 2, pw / 2, pw - pw / 2, h + ph, w + pw};
}

// out (2P, 3, hp, wp): images [0, P) from first[], [P, 2P) from second[]
__global__ __launch_bounds__(256) void fc_input(const uint8_t* __restrict__ frames, const int* __restrict__ first,
                                                const int* __restrict__ second, float* __restrict__ out, int n, int P,
                                                int h, int w, int top, int left, int hp, int wp) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * kFcBlock + threadIdx.x, y = blockIdx.y * kFcBlock + threadIdx.y;
    if (x >= wp || y >= hp) return;
    const int b = blockIdx.z;
    const int f = b < P ? first[b] : second[b - P];
    const size_t plane = size_t(hp) * wp, q = size_t(y) * wp + x;
    float* o = out + size_t(b) * 3 * plane + q;
    if (f < 0 || f >= n) {  // rejected on the host; never read outside the frames
        for (int c = 0; c < 3; ++c) o[c * plane] = __builtin_nanf("");
        return;
    }
    const int sy = min(max(y - top, 0), h - 1), sx = min(max(x - left, 0), w - 1);
    const uint8_t* px = frames + (size_t(f) * h * w + size_t(sy) * w + sx) * 3;
    const float inv255 = 1.0f / 255.0f;
    for (int c = 0; c < 3; ++c) {
        const float v = float(px[c]) * inv255;
        o[c * plane] = (v - kMean[c]) / kStd[c];
    }
}

// flows (2P, 2, hp, wp): pair n's fwd field at n, its bwd field at P + n
__global__ __launch_bounds__(256) void fc_output(const float* __restrict__ flows, float* __restrict__ bwd_flow,
                                                 uint8_t* __restrict__ bwd_occ, float* __restrict__ fwd_flow,
                                                 uint8_t* __restrict__ fwd_occ, int P, int h, int w, int top, int left,
                                                 int hp, int wp, float alpha, float beta) {
    const int x = blockIdx.x * kFcBlock + threadIdx.x, y = blockIdx.y * kFcBlock + threadIdx.y;
    if (x >= w || y >= h) return;
    const int n = blockIdx.z;
    const size_t pplane = size_t(hp) * wp, origin = size_t(top) * wp + left;
    const float* f = flows + size_t(n) * 2 * pplane + origin;
    const float* b = flows + (size_t(P) + n) * 2 * pplane + origin;
    const FbCheck fb = fb_check(f, b, pplane, wp, x, y, h, w, alpha, beta);
    const size_t hw = size_t(h) * w, q = size_t(y) * w + x, p = size_t(y) * wp + x;
    bwd_flow[size_t(n) * 2 * hw + q] = b[p];
    bwd_flow[size_t(n) * 2 * hw + hw + q] = b[pplane + p];
    bwd_occ[size_t(n) * hw + q] = fb.occ_b ? 255 : 0;
    if (fwd_flow) {
        fwd_flow[size_t(n) * 2 * hw + q] = f[p];
        fwd_flow[size_t(n) * 2 * hw + hw + q] = f[pplane + p];
        fwd_occ[size_t(n) * hw + q] = fb.occ_f ? 255 : 0;
    }
}

// shared limits: sides >= 2 (the warps divide by w - 1, h - 1), padded planes below 2^30 elements
int fc_size_args(int h, int w) {
    if (h < 1 || w < 1) return FRESCO_EINVAL;
    if (h < 2 || w < 2 || int64_t(h + 8) * (w + 8) > (int64_t(1) << 30)) return FRESCO_EUNSUPPORTED;
    return FRESCO_OK;
}

}  // namespace
}  // namespace fresco

extern "C" int fresco_flowcalc_input(const uint8_t* frames, const int* first, const int* second, float* out, int n,
                                     int P, int h, int w, void* stream) {
    using namespace fresco;
    if (!frames || !first || !second || !out || n < 1 || P < 1) return FRESCO_EINVAL;
    int rc = fc_size_args(h, w);
    if (rc != FRESCO_OK) return rc;
    if (2 * int64_t(P) > kFcMaxBatch) return FRESCO_EUNSUPPORTED;
    const Pads p = sintel_pads(h, w);
    const dim3 grid((p.wp + kFcBlock - 1) / kFcBlock, (p.hp + kFcBlock - 1) / kFcBlock, 2 * P);
    fc_input<<<grid, dim3(kFcBlock, kFcBlock), 0, as_stream(stream)>>>(frames, first, second, out, n, P, h, w, p.top,
                                                                        p.left, p.hp, p.wp);
    return check_launch();
}

extern "C" int fresco_flowcalc_output(const float* flows, float* bwd_flow, uint8_t* bwd_occ, float* fwd_flow,
                                      uint8_t* fwd_occ, int P, int h, int w, float alpha, float beta, void* stream) {
    using namespace fresco;
    if (!flows || !bwd_flow || !bwd_occ || P < 1 || (!fwd_flow) != (!fwd_occ)) return FRESCO_EINVAL;
    int rc = fc_size_args(h, w);
    if (rc != FRESCO_OK) return rc;
    if (P > kFcMaxBatch) return FRESCO_EUNSUPPORTED;
    const Pads p = sintel_pads(h, w);
    const dim3 grid((w + kFcBlock - 1) / kFcBlock, (h + kFcBlock - 1) / kFcBlock, P);
    fc_output<<<grid, dim3(kFcBlock, kFcBlock), 0, as_stream(stream)>>>(flows, bwd_flow, bwd_occ, fwd_flow, fwd_occ, P,
                                                                         h, w, p.top, p.left, p.hp, p.wp, alpha, beta);
    return check_launch();
}
