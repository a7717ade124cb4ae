// gaussian_step.hip -- the model side of a training iteration in one pass: the parameter activations of GaussianModel
// (r2_gaussian/gaussian/gaussian_model.py:38-64, 112-126) and torch.optim.Adam over its four parameter groups
// (gaussian_model.py:188-215: betas (0.9, 0.999), eps 1e-15, no weight decay), replacing ~15 element-wise launches of the
// foreach optimizer plus the activation kernels and their autograd backward.
//
// One thread owns one Gaussian's 11 values (xyz 3, density 1, scaling 3, rotation 4): the rotation row, whose normalize
// Jacobian couples its four components, stays in registers, and is moved as one 16-byte load / store.  Every float op is
// rounded on its own (built with -ffp-contract=off) in the order torch's CUDA kernels evaluate it, so the results are
// torch's up to the last-bit differences listed in INTEGRATION.md.
#include "r2_common.hpp"
#include "cloud_model.hpp"

namespace r2 {
namespace {

// torch casts the Python double hyper-parameters to the tensor's float type
constexpr float ADAM_W1 = (float)(1.0 - 0.9);     // exp_avg.lerp_(grad, 1 - beta1)
constexpr float ADAM_B2 = 0.999f;                 // exp_avg_sq.mul_(beta2)
constexpr float ADAM_W2 = (float)(1.0 - 0.999);   //           .addcmul_(grad, grad, value=1 - beta2)
constexpr float ADAM_EPS = 1e-15f;

struct Act {
    int bounded;          // scaling = sigmoid(x) * range + lo; else exp(x)
    float range, lo;      // float(hi - lo), float(lo): the scalars torch multiplies / adds
};

struct Group {
    float *param, *exp_avg, *exp_avg_sq;
    const float *grad;    // dL / d(activated parameter); NULL: the group is not stepped
    float step_size;      // float(lr / bias_correction1)
    float bc2_sqrt;       // float(sqrt(bias_correction2))
};

struct StepArgs {
    Group g[4];           // xyz, density, scaling, rotation
};

// the Adam update of one value (torch/optim/adam.py, non-fused and non-capturable: _single_tensor_adam / _multi_tensor_adam)
__device__ __forceinline__ void adam(float &p, float &m, float &v, float g, const Group &G)
{
    m = m + ADAM_W1 * (g - m);                    // lerp, weight < 0.5 branch
    v = v * ADAM_B2 + ADAM_W2 * g * g;
    const float denom = sqrtf(v) / G.bc2_sqrt + ADAM_EPS;
    p = p + -G.step_size * (m / denom);           // addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ float4 normalize4(float4 q, float &n, float &d)
{
    // the norm in double, rounded once: within half an ulp, so q / d stays within 2 ulp of torch's float32 normalize
    const double x = q.x, y = q.y, z = q.z, w = q.w;
    n = (float)sqrt(x * x + y * y + z * z + w * w);
    d = fmaxf(n, 1e-12f);                         // F.normalize: q / norm.clamp_min(eps)
    return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}

__global__ void __launch_bounds__(256) gaussian_activate_kernel(int P, const float *__restrict__ density,
                                                                const float *__restrict__ scaling,
                                                                const float *__restrict__ rotation, Act act,
                                                                float *__restrict__ density_act, float *__restrict__ scaling_act,
                                                                float *__restrict__ rotation_act)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    density_act[i] = softplus_f(density[i]);
    for (int k = 0; k < 3; ++k) scaling_act[3 * (size_t)i + k] = scale_act(scaling[3 * (size_t)i + k], act.bounded, act.range, act.lo);
    float n, d;
    reinterpret_cast<float4 *>(rotation_act)[i] = normalize4(reinterpret_cast<const float4 *>(rotation)[i], n, d);
}

__global__ void __launch_bounds__(256) gaussian_adam_kernel(int P, StepArgs s, Act act, float *__restrict__ density_act,
                                                            float *__restrict__ scaling_act, float *__restrict__ rotation_act)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i;

    // xyz: the identity activation
    if (const Group &G = s.g[0]; G.grad) {
        for (int k = 0; k < 3; ++k) {
            float p = G.param[i3 + k], m = G.exp_avg[i3 + k], v = G.exp_avg_sq[i3 + k];
            adam(p, m, v, G.grad[i3 + k], G);
            G.param[i3 + k] = p; G.exp_avg[i3 + k] = m; G.exp_avg_sq[i3 + k] = v;
        }
    }

    // density: softplus; softplus_backward: x > threshold ? g : g * z / (z + 1), z = exp(x)
    {
        const Group &G = s.g[1];
        float x = G.param[i];
        if (G.grad) {
            const float z = expf(x);
            const float g = x > 20.f ? G.grad[i] : G.grad[i] * z / (z + 1.0f);
            float m = G.exp_avg[i], v = G.exp_avg_sq[i];
            adam(x, m, v, g, G);
            G.param[i] = x; G.exp_avg[i] = m; G.exp_avg_sq[i] = v;
        }
        density_act[i] = softplus_f(x);
    }

    // scaling: sigmoid(x) * range + lo (mul backward, then sigmoid_backward g * (1 - y) * y), or exp(x) (g * exp(x))
    {
        const Group &G = s.g[2];
        for (int k = 0; k < 3; ++k) {
            float x = G.param[i3 + k];
            if (G.grad) {
                float g;
                if (act.bounded) {
                    const float y = sigmoid_f(x);
                    g = G.grad[i3 + k] * act.range * (1.0f - y) * y;
                } else {
                    g = G.grad[i3 + k] * expf(x);
                }
                float m = G.exp_avg[i3 + k], v = G.exp_avg_sq[i3 + k];
                adam(x, m, v, g, G);
                G.param[i3 + k] = x; G.exp_avg[i3 + k] = m; G.exp_avg_sq[i3 + k] = v;
            }
            scaling_act[i3 + k] = scale_act(x, act.bounded, act.range, act.lo);
        }
    }

    // rotation: q / max(|q|, eps).  autograd through div, clamp_min and norm:
    //   dq_j = g_j / d + q_j * (gn / n),  gn = [n >= eps] * sum_j -g_j * ((q_j / d) / d)   (= (g - q^(q^.g)) / |q| for |q| >= eps)
    {
        const Group &G = s.g[3];
        float4 q = reinterpret_cast<const float4 *>(G.param)[i];
        if (G.grad) {
            const float4 g = reinterpret_cast<const float4 *>(G.grad)[i];
            float n, d;
            normalize4(q, n, d);
            float gd = -g.x * ((q.x / d) / d);
            gd = gd + -g.y * ((q.y / d) / d);
            gd = gd + -g.z * ((q.z / d) / d);
            gd = gd + -g.w * ((q.w / d) / d);
            const float gn = n >= 1e-12f ? gd : 0.f;
            const float r = n == 0.f ? 0.f : gn / n;   // norm_backward is 0 where the norm is 0
            const float dq[4] = { g.x / d + q.x * r, g.y / d + q.y * r, g.z / d + q.z * r, g.w / d + q.w * r };
            float4 m = reinterpret_cast<const float4 *>(G.exp_avg)[i];
            float4 v = reinterpret_cast<const float4 *>(G.exp_avg_sq)[i];
            adam(q.x, m.x, v.x, dq[0], G);
            adam(q.y, m.y, v.y, dq[1], G);
            adam(q.z, m.z, v.z, dq[2], G);
            adam(q.w, m.w, v.w, dq[3], G);
            reinterpret_cast<float4 *>(G.param)[i] = q;
            reinterpret_cast<float4 *>(G.exp_avg)[i] = m;
            reinterpret_cast<float4 *>(G.exp_avg_sq)[i] = v;
        }
        float n, d;
        reinterpret_cast<float4 *>(rotation_act)[i] = normalize4(q, n, d);
    }
}

bool make_act(double lo, double hi, Act &a)
{
    if (lo == 0.0 && hi == 0.0) {
        a.bounded = 0; a.range = 0.f; a.lo = 0.f;
        return true;
    }
    if (!(lo < hi)) return false;                 // NaN included
    a.bounded = 1; a.range = (float)(hi - lo); a.lo = (float)lo;
    return true;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace r2

extern "C" int r2_gaussian_activate(int P, const float *density, const float *scaling, const float *rotation, double scale_lo,
                                    double scale_hi, float *density_act, float *scaling_act, float *rotation_act, void *stream)
{
    r2::Act act;
    if (P < 0 || !r2::make_act(scale_lo, scale_hi, act)) {
        r2::set_error("r2_gaussian_activate: invalid argument (P < 0, or a scale bound that is neither lo < hi nor 0, 0)");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    if (!density || !scaling || !rotation || !density_act || !scaling_act || !rotation_act || !r2::aligned16(rotation) ||
        !r2::aligned16(rotation_act)) {
        r2::set_error("r2_gaussian_activate: NULL array, or a rotation array that is not 16-byte aligned");
        return R2_ERR_INVALID;
    }
    r2::gaussian_activate_kernel<<<dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(
        P, density, scaling, rotation, act, density_act, scaling_act, rotation_act);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "gaussian activation");
    return 0;
}

extern "C" int r2_gaussian_adam_step(int P, float *const *params, const float *const *grads, float *const *exp_avg,
                                     float *const *exp_avg_sq, const double *lr, const double *bias_correction1,
                                     const double *bias_correction2, double scale_lo, double scale_hi, float *density_act,
                                     float *scaling_act, float *rotation_act, void *stream)
{
    r2::Act act;
    if (P < 0 || !params || !grads || !exp_avg || !exp_avg_sq || !lr || !bias_correction1 || !bias_correction2 ||
        !r2::make_act(scale_lo, scale_hi, act)) {
        r2::set_error("r2_gaussian_adam_step: invalid argument (P < 0, NULL pointer array, or a scale bound that is neither "
                      "lo < hi nor 0, 0)");
        return R2_ERR_INVALID;
    }
    r2::StepArgs s;
    for (int k = 0; k < 4; ++k) {
        r2::Group &G = s.g[k];
        G.param = params[k];
        G.grad = grads[k];
        G.exp_avg = G.grad ? exp_avg[k] : nullptr;
        G.exp_avg_sq = G.grad ? exp_avg_sq[k] : nullptr;
        G.step_size = G.bc2_sqrt = 0.f;
        if (G.grad) {
            if (!(bias_correction1[k] > 0.0) || !(bias_correction2[k] > 0.0) || !(lr[k] >= 0.0)) {
                r2::set_error("r2_gaussian_adam_step: group %d: lr must be >= 0 and both bias corrections > 0", k);
                return R2_ERR_INVALID;
            }
            G.step_size = (float)(lr[k] / bias_correction1[k]);
            G.bc2_sqrt = (float)sqrt(bias_correction2[k]);
        }
    }
    if (P == 0) return 0;
    bool ok = density_act && scaling_act && rotation_act && r2::aligned16(rotation_act);
    for (int k = 0; k < 4; ++k) {
        const r2::Group &G = s.g[k];
        ok = ok && G.param && (!G.grad || (G.exp_avg && G.exp_avg_sq));
        if (k == 3) ok = ok && r2::aligned16(G.param) && r2::aligned16(G.grad) && r2::aligned16(G.exp_avg) &&
                         r2::aligned16(G.exp_avg_sq);
    }
    if (!ok) {
        r2::set_error("r2_gaussian_adam_step: NULL parameter / moment / output array, or a rotation array that is not "
                      "16-byte aligned");
        return R2_ERR_INVALID;
    }
    r2::gaussian_adam_kernel<<<dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(P, s, act, density_act, scaling_act,
                                                                                          rotation_act);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "gaussian adam step");
    return 0;
}
