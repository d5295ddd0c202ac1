// reg_s4096.hip -- one size of the streamed single-frame kernels (the family is described at the top of reg_s1024.hip); a group of the kernel
// registry (rb_registry.hpp): ids are stable handles for tests and A/B runs (AGX_VARIANT_REGBLOCK_BASE + id), not indices.
#define AGX_TU tu_s4096
#include "rb_kernels.hpp"
#include "rb_stream_opts.hpp"

namespace agx {
namespace AGX_TU {
const rb_entry kEntries[] = {
    // n = 4096, FORWARD ONLY: 128 threads x 32 coefficients, frame loads at raised priority; the forward companion of the R = 3 default (id 93):
    // 59.5 vs 58.2 M NTT/s, 18.5 vs 18.9 uJ per NTT at the same 1400 W (profiles/r03_energy_ab.txt); its inverse (-1 %) and parked
    // product (-4 %) lose to id 93's, so only the forward kernel ships (A/B twin with all three transforms: id 147)
    make_entry_single_fwd<12, 5, kLazy | (kOptPrio << 1), 4>(159),
    // the same shape for plans whose moduli are all 2^60 - c, 0 < c < 2^28 (arithmetic level 3): the two-twiddle butterfly (six multiply-adds, a sign-bit
    // subtract on every stage but the first, slots {w, w 2^32 mod q} split at bit 29), final reduction by the top four bits; takes id 159's place as
    // the forward companion of such plans (ntt_kernels.hip: kCompanionDefaults).  Two kernels behind the id, one table: a plan whose moduli all have
    // c <= 2^27 (kQ60cSkipMaxC; the flag is the plan's, plan_view::q60c_skip) gets the skip form -- reduction by the top four bits on the even stages
    // only, 7q in place of 8q, any 64-bit input -- and every other plan, mixed ones included, the every-stage kernel above
    // Both kernels take the last conditional subtract once per wave instead of once per coefficient (kOptQ60cRareSub: a 32-bit compare per output feeds a
    // scalar mask, the subtract runs in a cold block behind one scalar branch) and address the per-lane table entries of passes 1 and 2 from a base
    // advanced on the scalar unit (kOptTwScalarBase); same words out, same table
    make_entry_single_fwd_q60c_skip<12, 5, kLazy | ((kOptPrio | kOptQ60c | kOptQ60cFold | kOptQ60cRareSub | kOptTwScalarBase) << 1), 4>(165),
#ifdef AGX_DIAG
    // A/B twins of id 165 (tools/energy_ab.py): the two kernels it launched before those two options (169), and with each option alone (170: the
    // rare subtract, 171: the scalar table bases)
    make_entry_single_fwd_q60c_skip<12, 5, kLazy | ((kOptPrio | kOptQ60c | kOptQ60cFold) << 1), 4>(169),
    make_entry_single_fwd_q60c_skip<12, 5, kLazy | ((kOptPrio | kOptQ60c | kOptQ60cFold | kOptQ60cRareSub) << 1), 4>(170),
    make_entry_single_fwd_q60c_skip<12, 5, kLazy | ((kOptPrio | kOptQ60c | kOptQ60cFold | kOptTwScalarBase) << 1), 4>(171),
    // A/B twin of id 165 that always launches the every-stage kernel, whatever the plan's moduli (tools/energy_ab.py)
    make_entry_single_fwd<12, 5, kLazy | ((kOptPrio | kOptQ60c | kOptQ60cFold) << 1), 4>(168),
    // A/B twin of id 165 with the butterfly it had before: quotient estimate from {w, w'}, sign-bit subtracts on the tail-free schedule (tools/energy_ab.py)
    make_entry_single_fwd<12, 5, kLazy | ((kOptPrio | kOptQ60c) << 1), 4>(167),
    // A/B twins kept in lib/libagxntt_diag.so: all three transforms in this shape with the load priority (147: its inverse -1 %, its parked
    // product -4 % against id 93's), and R = 4 streamed one table entry at a time at 8 waves/SIMD (161: equal to the default within 1 %)
    make_entry_single<12, 5, kLazy | (kOptPrio << 1), 4>(147),
    make_entry_single<12, 4, kLazy | (kOptStreamCh1 << 1), 8>(161),
#endif
};
}  // namespace AGX_TU

rb_span rb_entries_s4096() { return rb_span{AGX_TU::kEntries, sizeof(AGX_TU::kEntries) / sizeof(AGX_TU::kEntries[0])}; }

}  // namespace agx
