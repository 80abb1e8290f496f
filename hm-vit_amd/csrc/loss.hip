// The detector loss of the standalone PointPillar (opencood/loss/point_pillar_loss.py:68-142) with its gradient:
//
//   k_pp_count   per (sample, block) count of positive anchors (pos_equal_one > 0), written to the workspace
//   k_pp_loss    one thread per pixel of one sample: the block first sums its sample's counts (the normaliser max(1, #pos)),
//                then every anchor of the pixel gives its focal-loss term and its 7 smooth-L1 terms together with their
//                derivatives, written straight into dpsm / drm; per-block sums of the two loss terms go to the workspace
//   k_pp_final   one block: the per-block sums in a fixed order -> {conf_loss, reg_loss, total}
//
// A plain streaming pass (every input read once, every gradient written once).  No float atomics: a thread's terms, the block's
// LDS tree and the final sum all run in a fixed order (f64 accumulation), so two calls give the same bits.  The sigmoid / BCE
// forms take exp(-|x|) only, finite for logits of any magnitude.
#include "common.hpp"

namespace hmvit {

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 64;     // blocks per sample (grid-stride beyond): keeps the final sum short

inline int loss_blocks(int HW) { return HW <= 0 ? 1 : (cdiv(HW, kLossThreads) < kLossMaxBlocks ? cdiv(HW, kLossThreads) : kLossMaxBlocks); }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kLossThreads) void k_pp_count(const float* __restrict__ label, int n_anchor, int* __restrict__ counts) {
    __shared__ int sh[kLossThreads];
    const int b = blockIdx.y;
    const float* l = label + (size_t)b * n_anchor;
    int c = 0;
    for (int j = blockIdx.x * kLossThreads + threadIdx.x; j < n_anchor; j += gridDim.x * kLossThreads) c += l[j] > 0.f ? 1 : 0;
    c = block_sum(c, sh);
    if (threadIdx.x == 0) counts[b * gridDim.x + blockIdx.x] = c;
}

struct LossArgs {
    const float* psm;
    const float* rm;
    const float* label;
    const float* targets;
    float* dpsm;
    float* drm;
    const int* counts;
    double* partial;     // (B, blocks, 2): conf, reg
    int B, HW, A;
    float cls_weight, reg_coe, alpha, gamma, beta;
};

__global__ __launch_bounds__(kLossThreads) void k_pp_loss(LossArgs p) {
    __shared__ double shd[kLossThreads];
    __shared__ int s_norm;
    const int b = blockIdx.y, nblk = gridDim.x;
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < nblk; ++i) n += p.counts[b * nblk + i];
        s_norm = n;
    }
    __syncthreads();
    const float norm = fmaxf((float)s_norm, 1.f);
    const int A = p.A, HW = p.HW, A7 = 7 * A;
    const float cls_scale = p.cls_weight / (float)p.B;         // d total / d sum(cls terms)
    const float reg_scale = p.reg_coe / (float)p.B;
    const float inv_beta = 1.f / p.beta;
    double conf = 0.0, reg = 0.0;
    for (int pix = blockIdx.x * kLossThreads + threadIdx.x; pix < HW; pix += nblk * kLossThreads) {
        const size_t anchor0 = ((size_t)b * HW + pix) * A;      // (b, h, w, a = 0) in pos_equal_one's layout
        for (int a = 0; a < A; ++a) {
            const float t = p.label[anchor0 + a];
            const float cw = ((t == 0.f) ? 1.f : 0.f) + ((t > 0.f) ? 1.f : 0.f);
            const float wc = cw / norm;                           // cls_weights / clamp(pos_normalizer, 1)
            const float wr = ((t > 0.f) ? 1.f : 0.f) / norm;      // reg_weights / clamp(pos_normalizer, 1)

            // ---- sigmoid focal loss with logits ----
            const size_t ic = ((size_t)b * A + a) * HW + pix;
            const float x = p.psm[ic];
            const float e = expf(-fabsf(x));
            const float r = 1.f / (1.f + e);
            const float s = x >= 0.f ? r : e * r;                 // sigmoid(x)
            const float sc = x >= 0.f ? e * r : r;                // 1 - sigmoid(x)
            const float aw = t * p.alpha + (1.f - t) * (1.f - p.alpha);
            const float pt = t * sc + (1.f - t) * s;
            const float ptg = powf(pt, p.gamma);
            const float fw = aw * ptg;
            const float bce = fmaxf(x, 0.f) - x * t + log1pf(e);
            // torch's adjoints: clamp_min passes where x >= 0, |x| has derivative sgn(x) (0 at 0)
            const float sgn = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
            const float dbce = (x >= 0.f ? 1.f : 0.f) - t - sgn * e * r;
            const float dpt = (1.f - 2.f * t) * (sc * s);
            const float dptg = p.gamma == 0.f ? 0.f : p.gamma * powf(pt, p.gamma - 1.f);
            const float dterm = aw * dptg * dpt * bce + fw * dbce;
            conf += (double)(fw * bce * wc);
            p.dpsm[ic] = cls_scale * wc * dterm;

            // ---- smooth-L1 on the 7 deltas, sine difference on the yaw ----
            const float* tg = p.targets + ((size_t)b * HW + pix) * A7 + a * 7;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const size_t ir = ((size_t)b * A7 + a * 7 + k) * HW + pix;
                const float pv = p.rm[ir];
                const float tv = tg[k];
                float ps, ts, dps, dts;
                if (k == 6) {
                    const float sp = sinf(pv), cp = cosf(pv), st = sinf(tv), ct = cosf(tv);
                    ps = sp * ct;
                    ts = cp * st;
                    dps = cp * ct;
                    dts = -sp * st;
                } else {
                    ps = pv;
                    ts = tv;
                    dps = 1.f;
                    dts = 0.f;
                }
                if (isnan(ts)) {                                  // torch.where(isnan(target), pred, target)
                    ts = ps;
                    dts = dps;
                }
                const float diff = ps - ts;
                const float n = fabsf(diff);
                const bool quad = n < p.beta;
                const float loc = quad ? 0.5f * n * n * inv_beta : n - 0.5f * p.beta;
                const float dsgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                const float dloc = quad ? diff * inv_beta : dsgn;
                reg += (double)(loc * wr);
                p.drm[ir] = reg_scale * wr * dloc * (dps - dts);
            }
        }
    }
    conf = block_sum(conf, shd);
    reg = block_sum(reg, shd);
    if (threadIdx.x == 0) {
        double* out = p.partial + 2 * ((size_t)b * nblk + blockIdx.x);
        out[0] = conf;
        out[1] = reg;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_pp_final(const double* __restrict__ partial, int n, int B, float cls_weight,
                                                           float reg_coe, float* __restrict__ loss3) {
    __shared__ double shd[kLossThreads];
    double c = 0.0, r = 0.0;
    for (int i = threadIdx.x; i < n; i += kLossThreads) {
        c += partial[2 * i];
        r += partial[2 * i + 1];
    }
    c = block_sum(c, shd);
    r = block_sum(r, shd);
    if (threadIdx.x == 0) {
        const float conf = (float)(c / B) * cls_weight;          // cls_loss.sum() / B * cls_weight
        const float regl = (float)(r / B) * reg_coe;
        loss3[0] = conf;
        loss3[1] = regl;
        loss3[2] = regl + conf;
    }
}

size_t workspace_layout(int B, int HW, size_t* off_partial) {
    const size_t n = (size_t)B * loss_blocks(HW);
    *off_partial = align_up(n * sizeof(int), 256);
    return *off_partial + n * 2 * sizeof(double);
}

}  // namespace

}  // namespace hmvit

using namespace hmvit;

extern "C" size_t hmvit_pointpillar_loss_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) {
        set_error("pointpillar_loss_workspace_bytes: B, H, W must be positive");
        return 0;
    }
    size_t off;
    return workspace_layout(B, H * W, &off);
}

extern "C" int hmvit_pointpillar_loss(const float* psm, const float* rm, const float* pos_equal_one, const float* targets, int B,
                                      int H, int W, int A, float cls_weight, float reg_coe, float alpha, float gamma, float beta,
                                      float* loss3, float* dpsm, float* drm, void* workspace, size_t workspace_bytes, void* stream) {
    HMVIT_CHECK_ARG(psm && rm && pos_equal_one && targets && loss3 && dpsm && drm && workspace, "pointpillar_loss: null pointer");
    HMVIT_CHECK_ARG(B > 0 && H > 0 && W > 0 && A > 0 && (long long)H * W * A * 7 < (1ll << 31), "pointpillar_loss: bad shape");
    HMVIT_CHECK_ARG(beta > 0.f && gamma >= 0.f, "pointpillar_loss: beta must be > 0 and gamma >= 0");
    const int HW = H * W;
    size_t off_partial;
    const size_t need = workspace_layout(B, HW, &off_partial);
    HMVIT_CHECK_ARG(workspace_bytes >= need, "pointpillar_loss: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nblk = loss_blocks(HW);
    int* counts = reinterpret_cast<int*>(workspace);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + off_partial);
    hipLaunchKernelGGL(k_pp_count, dim3(nblk, B), dim3(kLossThreads), 0, st, pos_equal_one, HW * A, counts);
    HMVIT_CHECK_LAUNCH();
    LossArgs p;
    p.psm = psm; p.rm = rm; p.label = pos_equal_one; p.targets = targets; p.dpsm = dpsm; p.drm = drm;
    p.counts = counts; p.partial = partial;
    p.B = B; p.HW = HW; p.A = A;
    p.cls_weight = cls_weight; p.reg_coe = reg_coe; p.alpha = alpha; p.gamma = gamma; p.beta = beta;
    hipLaunchKernelGGL(k_pp_loss, dim3(nblk, B), dim3(kLossThreads), 0, st, p);
    HMVIT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_pp_final, dim3(1), dim3(kLossThreads), 0, st, partial, B * nblk, B, cls_weight, reg_coe, loss3);
    HMVIT_CHECK_LAUNCH();
    return HMVIT_OK;
}
