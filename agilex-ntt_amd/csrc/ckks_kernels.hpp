// ckks_kernels.hpp -- the kernels of agx_ntt_ckks_encode (ckks_encode_kernel) and agx_ntt_ckks_decode (ckks_decode_kernel).  Compiled in ntt_kernels.hip.
// One workgroup per frame.  The special FFT of s = 2^log_s complex slots runs in register-blocked radix-2^R passes (R <= 3: a thread holds 2^R complex
// values at stride 2^p, does R stages on them and puts them back: rb_frame.hpp's shape, here with a run-time p), a workgroup barrier between passes.  The
// values between passes live in LDS as two planes of s doubles, real and imaginary apart (8-byte lanes on consecutive addresses), 16 s bytes: up to
// s = 8192 (128 KiB).  s = 16384 (n = 32768 with full slots, 256 KiB) takes the GLOBAL route: the same passes exchange through the frame's own output
// words -- decode's d_z frame (s pairs of doubles), encode's frame of slab 0 (n words = s pairs of doubles) --, which the workgroup alone touches; encode
// then moves every component off those words (the real ones into LDS, 16 imaginary ones per thread into registers), passes one more barrier, and only then
// writes the residues over them.
// The radix-2 data-flow graph fixes every rounding, so how the stages are grouped into passes does not change a bit.  ckks_arith.hpp has the per-word steps.
#pragma once
#include "ntt_kernels.hpp"
#include "ckks_arith.hpp"

namespace agx {

struct ckks_lds_planes {
    double *re, *im;
    __device__ __forceinline__ ckks_cplx get(uint32_t k) const { return {re[k], im[k]}; }
    __device__ __forceinline__ void put(uint32_t k, ckks_cplx c) const { re[k] = c.re, im[k] = c.im; }
};

struct ckks_global_planes {
    double2* p;
    __device__ __forceinline__ ckks_cplx get(uint32_t k) const { const double2 v = p[k]; return {v.x, v.y}; }
    __device__ __forceinline__ void put(uint32_t k, ckks_cplx c) const { p[k] = make_double2(c.re, c.im); }
};

__device__ __forceinline__ uint32_t ckks_bitrev(uint32_t k, uint32_t bits) { return bits ? __brev(k) >> (32u - bits) : 0u; }

// R stages on the values at stride 2^p: half-lengths 2^p ... 2^(p + R - 1), ascending for decode (INVERSE = false), descending for encode.  Group g of the
// s >> R groups holds the indices base + (m << p), m < 2^R, base = g with R zero bits put in at bit p.  In the stage of half-length h = 2^(p + r), value a
// (bit r of a clear) meets a | 1 << r under tw(2h, j), j = its index modulo h, at tw[h + j].
template <bool INVERSE, int R, class S>
__device__ __forceinline__ void ckks_pass(const S& st, const double2* __restrict__ tw, uint32_t p, uint32_t log_s) {
    constexpr int M = 1 << R;
    const uint32_t groups = (1u << log_s) >> R;
    for (uint32_t g = threadIdx.x; g < groups; g += blockDim.x) {
        const uint32_t base = ((g >> p) << (p + R)) | (g & ((1u << p) - 1u));
        ckks_cplx v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] = st.get(base + ((uint32_t)m << p));
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int r = INVERSE ? R - 1 - rr : rr;
            const uint32_t half = 1u << (p + r);
#pragma unroll
            for (int a = 0; a < M; ++a)
                if (!((a >> r) & 1)) {
                    const int b = a | (1 << r);
                    const double2 w = tw[half + ((base + ((uint32_t)a << p)) & (half - 1u))];
                    if (INVERSE) ckks_bfly_inv(v[a], v[b], ckks_cplx{w.x, w.y});
                    else ckks_bfly_fwd(v[a], v[b], ckks_cplx{w.x, w.y});
                }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) st.put(base + ((uint32_t)m << p), v[m]);
    }
}

// every stage, three to a pass while three are left, a barrier behind each pass
template <bool INVERSE, class S>
__device__ __forceinline__ void ckks_fft(const S& st, const double2* __restrict__ tw, uint32_t log_s) {
    for (uint32_t done = 0; done < log_s;) {
        const uint32_t R = log_s - done < 3u ? log_s - done : 3u;
        const uint32_t p = INVERSE ? log_s - done - R : done;
        if (R == 3) ckks_pass<INVERSE, 3>(st, tw, p, log_s);
        else if (R == 2) ckks_pass<INVERSE, 2>(st, tw, p, log_s);
        else ckks_pass<INVERSE, 1>(st, tw, p, log_s);
        __syncthreads();
        done += R;
    }
}

// what both kernels read of a handle and a call
struct ckks_args {
    const double2* tw;        // [n / 2] tw(len, j) at len / 2 + j
    const uint64_t* q;        // [L]
    const uint64_t* tri;      // Garner's pairs, two words each (ckks_arith.hpp)
    const uint64_t* pow2;     // [L][kCkksPow2] pairs, two words each
    uint32_t log_n, log_s, L;
    uint64_t per_prime;       // batch * n: the words of a slab
};

template <bool GLOBAL>
__device__ __forceinline__ auto ckks_planes(double2* global_frame, uint32_t s) {
    if constexpr (GLOBAL) return ckks_global_planes{global_frame};
    else {
        extern __shared__ __attribute__((aligned(16))) unsigned char agx_dyn_lds[];
        double* re = reinterpret_cast<double*>(agx_dyn_lds);
        return ckks_lds_planes{re, re + s};
    }
}

// agx_ntt_ckks_decode behind the inverse transform: x dense [L][batch][n] fully reduced -> z dense [batch][s] pairs.  A thread turns the L residues of
// coefficient k gap and of (k + s) gap into the doubles (x_k, x_{k+s}) (Garner, sign, Horner), stores them bit-reversed; the forward passes; one product by
// 1 / Delta per component.  8 n L bytes read where gap = 1 (the coefficients off the gap grid are never read), 16 s written.  GLOBAL: s = 16384, see above.
template <int SMAX, bool GLOBAL>
__global__ __launch_bounds__(1024) void ckks_decode_kernel(const uint64_t* __restrict__ x, double2* __restrict__ z, ckks_args a, double inv_delta) {
    const uint32_t s = 1u << a.log_s, gap_log = a.log_n - 1u - a.log_s;
    const uint64_t f = blockIdx.x;
    double2* zf = z + (f << a.log_s);
    const auto st = ckks_planes<GLOBAL>(zf, s);
    const uint64_t* xf = x + (f << a.log_n);
    for (uint32_t k = threadIdx.x; k < s; k += blockDim.x) {
        uint64_t xr[SMAX], xi[SMAX];
#pragma unroll
        for (int i = 0; i < SMAX; ++i) {
            xr[i] = xi[i] = 0;
            if ((uint32_t)i < a.L) {
                xr[i] = xf[(uint64_t)i * a.per_prime + ((uint64_t)k << gap_log)];
                xi[i] = xf[(uint64_t)i * a.per_prime + ((uint64_t)(k + s) << gap_log)];
            }
        }
        const double re = ckks_rns_to_double<SMAX>(xr, a.L, a.q, a.tri), im = ckks_rns_to_double<SMAX>(xi, a.L, a.q, a.tri);
        st.put(ckks_bitrev(k, a.log_s), ckks_cplx{re, im});
    }
    __syncthreads();
    ckks_fft<false>(st, a.tw, a.log_s);
    for (uint32_t k = threadIdx.x; k < s; k += blockDim.x) {
        const ckks_cplx c = st.get(k);
        zf[k] = make_double2(c.re * inv_delta, c.im * inv_delta);
    }
}

// one coefficient of encode: the component of w (1 / s applied, exact) -> x = fl(Delta component) -> c = rint(x) -> its residue under each of the L primes
__device__ __forceinline__ void ckks_store_residues(uint64_t* __restrict__ of, uint32_t idx, bool on_grid, double comp, double delta, double inv_s, const ckks_args& a) {
    bool negative = false;
    uint32_t e = 0;
    const uint64_t mant = on_grid ? ckks_round(delta * (comp * inv_s), &negative, &e) : 0;
    for (uint32_t i = 0; i < a.L; ++i) {
        const uint64_t* pw = a.pow2 + 2 * ((uint64_t)i * kCkksPow2 + e);
        of[(uint64_t)i * a.per_prime + idx] = ckks_residue(mant, negative, pw[0], pw[1], a.q[i]);
    }
}

// agx_ntt_ckks_encode in coefficient form: z dense [batch][s] pairs -> out dense [L][batch][n], fully reduced.  The slots go into the planes in natural order;
// the inverse passes; then one thread per coefficient index: index kk gap holds component kk < s ? Re : Im of v[bitrev(kk mod s)], every other index 0.
// 16 s bytes read, 8 n L written.  GLOBAL: s = 16384, n = 32768, 1024 threads, 8 s bytes of LDS, see above.
template <bool GLOBAL>
__global__ __launch_bounds__(1024) void ckks_encode_kernel(const double2* __restrict__ z, uint64_t* __restrict__ out, ckks_args a, double delta, double inv_s) {
    const uint32_t s = 1u << a.log_s, n = 1u << a.log_n, gap_log = a.log_n - 1u - a.log_s;
    const uint64_t f = blockIdx.x;
    uint64_t* of = out + (f << a.log_n);
    const auto st = ckks_planes<GLOBAL>(reinterpret_cast<double2*>(of), s);
    const double2* zf = z + (f << a.log_s);
    for (uint32_t k = threadIdx.x; k < s; k += blockDim.x) {
        const double2 v = zf[k];
        st.put(k, ckks_cplx{v.x, v.y});
    }
    __syncthreads();
    ckks_fft<true>(st, a.tw, a.log_s);
    if constexpr (GLOBAL) {
        // every value leaves the frame's words before the first residue lands on them: the real components wait in LDS (s doubles, each read back by the
        // thread that wrote it), the imaginary ones in registers
        constexpr int PER = 16;      // s / blockDim.x
        extern __shared__ __attribute__((aligned(16))) unsigned char agx_dyn_lds[];
        double* re = reinterpret_cast<double*>(agx_dyn_lds);
        double im[PER];
#pragma unroll
        for (int m = 0; m < PER; ++m) {
            const uint32_t k = threadIdx.x + (uint32_t)m * 1024u;
            const ckks_cplx c = st.get(ckks_bitrev(k, a.log_s));
            re[k] = c.re, im[m] = c.im;
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < s; k += 1024u) ckks_store_residues(of, k, true, re[k], delta, inv_s, a);
#pragma unroll
        for (int m = 0; m < PER; ++m) ckks_store_residues(of, s + threadIdx.x + (uint32_t)m * 1024u, true, im[m], delta, inv_s, a);
    } else {
        for (uint32_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
            const uint32_t kk = idx >> gap_log;
            const bool on_grid = (idx & ((1u << gap_log) - 1u)) == 0;
            double comp = 0.0;
            if (on_grid) {
                const ckks_cplx c = st.get(ckks_bitrev(kk & (s - 1u), a.log_s));
                comp = kk >= s ? c.im : c.re;
            }
            ckks_store_residues(of, idx, on_grid, comp, delta, inv_s, a);
        }
    }
}

}  // namespace agx
