// Fused elementwise halves of one EDM-Euler denoise step of the GEN3C sampler
// (cosmos_predict1/diffusion/model/model_v2w.py:130-149, 201-259; diffusers 0.32.2 EDMEulerScheduler).
//
// The reference runs ~25 separate bf16/fp32 elementwise torch kernels per step over the [B,16,T,88,160] latent.
// Here each side of the two network calls is ONE pass: (1) build the network input, (2) CFG + conditioning-frame
// replacement + Euler update. bf16 roundings are placed exactly where the reference's dtype promotion puts them
// (comments name the torch expression each rounding belongs to); scalar coefficients are computed by the host in
// the dtypes the reference uses and arrive as floats. "Where the reference puts them" includes WHERE each operand lives:
// the model's sigma is a bf16 0-dim tensor on the device, the scheduler's scalars are fp32 0-dim tensors on the CPU, and
// torch's device kernels take a CPU 0-dim operand as an fp32 scalar argument - unrounded in a product with a bf16 tensor,
// and as its host-computed reciprocal in a division. tests/sampler_ref.py is the statement of this dtype chain;
// tests/test_sampler_kernels_gpu.py holds both kernels to it bit for bit (built with -ffp-contract=off: no FMA where
// torch runs a multiply and an add as two kernels).
#include "common.hpp"

#include <cfloat>

namespace {

G3_DEVICE float rbf(float v) { return (float)f32_to_bf16(v); }  // one bf16 rounding

struct PrepArgs {
    const bf16_t* xt;        // current sample (bf16)
    const bf16_t* gt_latent; // condition.gt_latent (bf16)
    const float* noise;      // arch_invariant_rand(seed) fp32
    const float* indicator;  // [T] 0/1 per latent frame (already zeroed by the host when augment_sigma >= sigma)
    bf16_t* new_xt;          // model_v2w.py:138
    bf16_t* new_xt_scaled;   // model_v2w.py:139
    int64_t n; int T; int hw;
    float augment_sigma;     // condition_augment_sigma
    float c_in_aug;          // 1/sqrt(augment_sigma^2 + sigma_data^2)            (python floats, fp32 tensor math)
    float inv_c_in_bf16;     // divisor c_in of _reverse_precondition_input, evaluated in bf16 (sigma is a bf16 tensor)
    float c_in_step;         // scheduler.scale_model_input: 1/sqrt(sigma^2 + sigma_data^2) in fp32
};

__global__ __launch_bounds__(256) void edm_prepare_kernel(PrepArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const int t = (int)((i / a.hw) % a.T);
        const float ind = a.indicator[t];
        const float x = (float)a.xt[i];
        float v = x;
        if (ind != 0.f) {
            // augment_latent = latent + noise * augment_sigma                      (fp32)
            float al = (float)a.gt_latent[i] + a.noise[i] * a.augment_sigma;
            al = al * a.c_in_aug;            // scheduler.precondition_inputs       (fp32)
            al = al / a.inv_c_in_bf16;       // xt / c_in, c_in a bf16 0-dim tensor (fp32 result)
            v = ind * al + (1.f - ind) * x;  // model_v2w.py:246                    (fp32)
        }
        const bf16_t nx = f32_to_bf16(v);    // new_xt.to(bf16)
        a.new_xt[i] = nx;
        a.new_xt_scaled[i] = f32_to_bf16((float)nx * a.c_in_step);  // bf16 tensor * fp32 0-dim -> bf16
    }
}

struct StepArgs {
    const bf16_t* out_cond; const bf16_t* out_uncond;
    const bf16_t* new_xt; const bf16_t* gt_latent; const float* indicator;
    bf16_t* xt_next;
    int64_t n; int T; int hw;
    float guidance;
    float c_skip_bf16, c_out_bf16;  // _reverse_precondition_output coefficients, evaluated in bf16 (sigma bf16 tensor)
    float c_skip, c_out;            // scheduler.precondition_outputs coefficients (fp32 sigma)
    float sigma, sigma_next;        // fp32
    float inv_sigma;                // fp32 1 / sigma, divided on the host
};

__global__ __launch_bounds__(256) void edm_step_kernel(StepArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const int t = (int)((i / a.hw) % a.T);
        const float ind = a.indicator[t];
        const float oc = (float)a.out_cond[i], ou = (float)a.out_uncond[i];
        // net_output = cond + guidance * (cond - uncond)          three bf16 tensor ops (model_v2w.py:144)
        float no = rbf(oc + rbf(a.guidance * rbf(oc - ou)));
        const float x = (float)a.new_xt[i];
        if (ind != 0.f) {
            // latent_unscaled = (latent - c_skip * xt) / c_out     bf16 tensor ops (model_v2w.py:254-259)
            const float lu = rbf(rbf((float)a.gt_latent[i] - rbf(a.c_skip_bf16 * x)) / a.c_out_bf16);
            // new_output = indicator * latent_unscaled + (1 - indicator) * net_output   (bf16, :147)
            no = rbf(rbf(ind * lu) + rbf(rbf(1.f - ind) * no));
        }
        // EDMEulerScheduler.step: sample upcast to fp32; c_out * model_output is a bf16 product whose fp32 CPU 0-dim factor is not rounded
        const float x0 = a.c_skip * x + rbf(a.c_out * no);
        // (sample - x0) / sigma_hat with a CPU 0-dim divisor: torch's device kernel multiplies by the reciprocal taken on the host
        const float deriv = (x - x0) * a.inv_sigma;
        a.xt_next[i] = f32_to_bf16(x + deriv * (a.sigma_next - a.sigma));  // prev_sample.to(model_output.dtype)
    }
}

// The opt-in second-order multistep solver ("2ab": the Adams-Bashforth exponential integrator of arXiv 2308.02157, the reference's
// functional/multi_step.py::order2_fn). Everything up to and including the fp32 x0 prediction is edm_step_kernel's chain, restated here so that
// the Euler kernel stays as it is; the x0 prediction is also stored (fp32) as the next step's history. have_prev == 0: the Euler update, the same
// bits as edm_step_kernel. have_prev != 0: xt_next = bf16(a * x + (cb1 * x0 + cb2 * x0_prev)), each an fp32 operation of its own (no contraction),
// a / cb1 / cb2 computed by the host in fp64 (gen3c_amd/sampler.py::res_2ab_coefficients). x0_out may be x0_prev: element i is read before it is
// written, by the one thread that owns it. Plain 4-byte history accesses: the kernel moves 18 B per element once per 3 s step.
struct Step2abArgs {
    StepArgs e;
    const float* x0_prev; float* x0_out;
    int have_prev;
    float a, cb1, cb2;
};

__global__ __launch_bounds__(256) void edm_step_2ab_kernel(Step2abArgs s) {
    const StepArgs& a = s.e;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const int t = (int)((i / a.hw) % a.T);
        const float ind = a.indicator[t];
        const float oc = (float)a.out_cond[i], ou = (float)a.out_uncond[i];
        float no = rbf(oc + rbf(a.guidance * rbf(oc - ou)));
        const float x = (float)a.new_xt[i];
        if (ind != 0.f) {
            const float lu = rbf(rbf((float)a.gt_latent[i] - rbf(a.c_skip_bf16 * x)) / a.c_out_bf16);
            no = rbf(rbf(ind * lu) + rbf(rbf(1.f - ind) * no));
        }
        const float x0 = a.c_skip * x + rbf(a.c_out * no);
        float next;
        if (s.have_prev) {
            const float hist = s.cb1 * x0 + s.cb2 * s.x0_prev[i];  // read before x0_out[i] is written: the two may be one buffer
            next = s.a * x + hist;
        } else {
            const float deriv = (x - x0) * a.inv_sigma;
            next = x + deriv * (a.sigma_next - a.sigma);
        }
        s.x0_out[i] = x0;
        a.xt_next[i] = f32_to_bf16(next);
    }
}

// The opt-in guidance interval (classifier-free guidance only while sigma_lo < sigma <= sigma_hi, arXiv 2404.07724): a step outside the interval has
// no unconditional network output, net_output IS out_cond (no arithmetic on it). From the conditioning-frame replacement on, the chain of
// edm_step_kernel / edm_step_2ab_kernel restated - the same bf16 rounding points, the same fp32 operations - so that those two kernels stay as they
// are. cond_x0 is shared by the two kernels below and by nothing else.
struct CondStepArgs {
    const bf16_t* out_cond;
    const bf16_t* new_xt; const bf16_t* gt_latent; const float* indicator;
    bf16_t* xt_next;
    int64_t n; int T; int hw;
    float c_skip_bf16, c_out_bf16;
    float c_skip, c_out;
    float sigma, sigma_next;
    float inv_sigma;
};

G3_DEVICE float cond_x0(const CondStepArgs& a, int64_t i, float x) {
    const int t = (int)((i / a.hw) % a.T);
    const float ind = a.indicator[t];
    float no = (float)a.out_cond[i];  // net_output = out_cond
    if (ind != 0.f) {
        const float lu = rbf(rbf((float)a.gt_latent[i] - rbf(a.c_skip_bf16 * x)) / a.c_out_bf16);
        no = rbf(rbf(ind * lu) + rbf(rbf(1.f - ind) * no));
    }
    return a.c_skip * x + rbf(a.c_out * no);
}

__global__ __launch_bounds__(256) void edm_cond_step_kernel(CondStepArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const float x = (float)a.new_xt[i];
        const float x0 = cond_x0(a, i, x);
        const float deriv = (x - x0) * a.inv_sigma;
        a.xt_next[i] = f32_to_bf16(x + deriv * (a.sigma_next - a.sigma));
    }
}

struct CondStep2abArgs {
    CondStepArgs e;
    const float* x0_prev; float* x0_out;
    int have_prev;
    float a, cb1, cb2;
};

__global__ __launch_bounds__(256) void edm_cond_step_2ab_kernel(CondStep2abArgs s) {
    const CondStepArgs& a = s.e;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const float x = (float)a.new_xt[i];
        const float x0 = cond_x0(a, i, x);
        float next;
        if (s.have_prev) {
            const float hist = s.cb1 * x0 + s.cb2 * s.x0_prev[i];  // read before x0_out[i] is written: the two may be one buffer
            next = s.a * x + hist;
        } else {
            const float deriv = (x - x0) * a.inv_sigma;
            next = x + deriv * (a.sigma_next - a.sigma);
        }
        s.x0_out[i] = x0;
        a.xt_next[i] = f32_to_bf16(next);
    }
}

int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b > 256 * 8 ? 256 * 8 : b);
}

}  // namespace

extern "C" int g3_edm_prepare_input_bf16(const void* xt, const void* gt_latent, const float* noise,
                                         const float* indicator, void* new_xt, void* new_xt_scaled, int64_t n, int T,
                                         int hw, float augment_sigma, float c_in_aug, float c_in_bf16, float c_in_step,
                                         void* stream) {
    if (!xt || !gt_latent || !noise || !indicator || !new_xt || !new_xt_scaled)
        return g3_set_error(G3_ERR_ARG, "g3_edm_prepare_input_bf16: null operand");
    if (n <= 0 || T <= 0 || hw <= 0) return g3_set_error(G3_ERR_ARG, "g3_edm_prepare_input_bf16: bad shape");
    PrepArgs a{(const bf16_t*)xt, (const bf16_t*)gt_latent, noise, indicator, (bf16_t*)new_xt, (bf16_t*)new_xt_scaled,
               n, T, hw, augment_sigma, c_in_aug, c_in_bf16, c_in_step};
    hipLaunchKernelGGL(edm_prepare_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a);
    return g3_check_launch("g3_edm_prepare_input_bf16");
}

extern "C" int g3_edm_cfg_euler_step_bf16(const void* out_cond, const void* out_uncond, const void* new_xt,
                                          const void* gt_latent, const float* indicator, void* xt_next, int64_t n,
                                          int T, int hw, float guidance, float c_skip_bf16, float c_out_bf16,
                                          float c_skip, float c_out, float sigma, float inv_sigma, float sigma_next,
                                          void* stream) {
    if (!out_cond || !out_uncond || !new_xt || !gt_latent || !indicator || !xt_next)
        return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_euler_step_bf16: null operand");
    if (n <= 0 || T <= 0 || hw <= 0 || sigma <= 0.f || !(inv_sigma > 0.f)) return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_euler_step_bf16: bad argument");
    StepArgs a{(const bf16_t*)out_cond, (const bf16_t*)out_uncond, (const bf16_t*)new_xt, (const bf16_t*)gt_latent,
               indicator, (bf16_t*)xt_next, n, T, hw, guidance, c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, sigma_next, inv_sigma};
    hipLaunchKernelGGL(edm_step_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a);
    return g3_check_launch("g3_edm_cfg_euler_step_bf16");
}

extern "C" int g3_edm_cfg_2ab_step_bf16(const void* out_cond, const void* out_uncond, const void* new_xt, const void* gt_latent,
                                        const float* indicator, void* xt_next, int64_t n, int T, int hw, float guidance,
                                        float c_skip_bf16, float c_out_bf16, float c_skip, float c_out, float sigma, float inv_sigma,
                                        float sigma_next, const float* x0_prev, float* x0_out, int have_prev, float a, float cb1,
                                        float cb2, void* stream) {
    if (!out_cond || !out_uncond || !new_xt || !gt_latent || !indicator || !xt_next || !x0_out)
        return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_2ab_step_bf16: null operand");
    if (n <= 0 || T <= 0 || hw <= 0 || sigma <= 0.f || !(inv_sigma > 0.f)) return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_2ab_step_bf16: bad argument");
    if (have_prev && !x0_prev) return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_2ab_step_bf16: have_prev without x0_prev");
    if (have_prev && !(a > 0.f && a <= FLT_MAX)) return g3_set_error(G3_ERR_ARG, "g3_edm_cfg_2ab_step_bf16: a must be finite and positive");
    Step2abArgs s{{(const bf16_t*)out_cond, (const bf16_t*)out_uncond, (const bf16_t*)new_xt, (const bf16_t*)gt_latent, indicator,
                   (bf16_t*)xt_next, n, T, hw, guidance, c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, sigma_next, inv_sigma},
                  x0_prev, x0_out, have_prev, a, cb1, cb2};
    hipLaunchKernelGGL(edm_step_2ab_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, s);
    return g3_check_launch("g3_edm_cfg_2ab_step_bf16");
}

extern "C" int g3_edm_cond_euler_step_bf16(const void* out_cond, const void* new_xt, const void* gt_latent, const float* indicator,
                                           void* xt_next, int64_t n, int T, int hw, float c_skip_bf16, float c_out_bf16, float c_skip,
                                           float c_out, float sigma, float inv_sigma, float sigma_next, void* stream) {
    if (!out_cond || !new_xt || !gt_latent || !indicator || !xt_next)
        return g3_set_error(G3_ERR_ARG, "g3_edm_cond_euler_step_bf16: null operand");
    if (n <= 0 || T <= 0 || hw <= 0 || sigma <= 0.f || !(inv_sigma > 0.f)) return g3_set_error(G3_ERR_ARG, "g3_edm_cond_euler_step_bf16: bad argument");
    CondStepArgs a{(const bf16_t*)out_cond, (const bf16_t*)new_xt, (const bf16_t*)gt_latent, indicator, (bf16_t*)xt_next, n, T, hw,
                   c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, sigma_next, inv_sigma};
    hipLaunchKernelGGL(edm_cond_step_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a);
    return g3_check_launch("g3_edm_cond_euler_step_bf16");
}

extern "C" int g3_edm_cond_2ab_step_bf16(const void* out_cond, const void* new_xt, const void* gt_latent, const float* indicator,
                                         void* xt_next, int64_t n, int T, int hw, float c_skip_bf16, float c_out_bf16, float c_skip,
                                         float c_out, float sigma, float inv_sigma, float sigma_next, const float* x0_prev, float* x0_out,
                                         int have_prev, float a, float cb1, float cb2, void* stream) {
    if (!out_cond || !new_xt || !gt_latent || !indicator || !xt_next || !x0_out)
        return g3_set_error(G3_ERR_ARG, "g3_edm_cond_2ab_step_bf16: null operand");
    if (n <= 0 || T <= 0 || hw <= 0 || sigma <= 0.f || !(inv_sigma > 0.f)) return g3_set_error(G3_ERR_ARG, "g3_edm_cond_2ab_step_bf16: bad argument");
    if (have_prev && !x0_prev) return g3_set_error(G3_ERR_ARG, "g3_edm_cond_2ab_step_bf16: have_prev without x0_prev");
    if (have_prev && !(a > 0.f && a <= FLT_MAX)) return g3_set_error(G3_ERR_ARG, "g3_edm_cond_2ab_step_bf16: a must be finite and positive");
    CondStep2abArgs s{{(const bf16_t*)out_cond, (const bf16_t*)new_xt, (const bf16_t*)gt_latent, indicator, (bf16_t*)xt_next, n, T, hw,
                       c_skip_bf16, c_out_bf16, c_skip, c_out, sigma, sigma_next, inv_sigma},
                      x0_prev, x0_out, have_prev, a, cb1, cb2};
    hipLaunchKernelGGL(edm_cond_step_2ab_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, s);
    return g3_check_launch("g3_edm_cond_2ab_step_bf16");
}
