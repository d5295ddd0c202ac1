// moddown_coeff_body.hpp -- the body of moddown_coeff_kernel (AGX_RESCALE_FLOOR) and moddown_coeff_round_kernel (AGX_RESCALE_ROUND), ntt_kernels.hip: ONE
// text, included inside both kernels' braces, for the reason moddown_rb2_body.hpp gives (FLOOR keeps the assembly it had).  No include guard, nothing at
// namespace scope.  The including kernel has the template parameter SMAX, the arguments out, y, dst_consts, mat, dall, S, T, per_prime, and in scope
//   constexpr bool ROUND;  const ulonglong2* rsrc ([S] {c_i, q_i});  const uint64_t* rdst ([T] t h mod q_j)
// -- arguments of the ROUND kernel, constant null pointers in the FLOOR kernel, where no statement that names them is instantiated.
for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t yi[SMAX];
#pragma unroll
    for (int i = 0; i < SMAX; ++i)
        if ((uint32_t)i < S) {
            yi[i] = y[(uint64_t)i * per_prime + e];
            if constexpr (ROUND) {
                const ulonglong2 rs = rsrc[i];      // {c_i, q_i}
                yi[i] = moddown_round_y(yi[i], rs.x, rs.y);
            }
        }
    for (uint32_t j = 0; j < T; ++j) {
        const uint64_t q = dst_consts[j].q, q2 = q << 1;
        const ulonglong2* row = mat + (size_t)j * S;
        const ulonglong2 d = dall[j];
        uint64_t acc = 0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if ((uint32_t)i < S) {
                const ulonglong2 c = row[i];
                acc = basis_accumulate(acc, yi[i], c.x, c.y, q, q2);
            }
        if constexpr (ROUND) acc = moddown_round_acc(acc, rdst[j], q);
        uint64_t* o = out + (uint64_t)j * per_prime + e;
        *o = rescale_finish<false>(*o, csub(acc, q), d.x, d.y, q);
    }
}
