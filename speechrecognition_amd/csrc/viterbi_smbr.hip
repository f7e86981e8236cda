// viterbi_smbr.hip -- the kernels of sMBR training over the recognition network (viterbi_netfb.hip's network, scale kappa, penalties
// and start hypothesis): beside alpha and beta, the expected number of correctly labelled frames of the paths through every (frame,
// position), and from it the signed weights gamma_t(k) = occ_t(k) (c_t(k) - Abar) = -(1 / kappa) d Abar / d e(t, k).
//
// Accuracy.  A path scores 1 at frame t when the mixture whose emission it pays there is ref[t]; an entry into position 1 of a word
// pays the word's FIRST state (the reference's quirk, as in viterbi_mmi.hip) and is scored as that state.  ref[t] >= the state count
// matches no slot.
//
//   smbr_forward_kernel    alpha_t(s) as netfb_forward_kernel, and abar_t(s) = the expected accuracy of frames 0 .. t over the paths
//                          reaching s at t, in the linear domain: the mean of the sources' abar_{t-1} plus the accuracy of the emission
//                          taken, weighted with exp(alpha_t(s) - term).  The word-end reduction carries sum exp(m - x) abar beside
//                          (min m, sum exp(m - x)): E_t and Ebar_t are kept per frame; kappa F_u = E_{T-1}, Abar_u = Ebar_{T-1}.
//   smbr_backward_kernel   beta_t(s) and bbar_t(s) = the expected accuracy of frames t + 1 .. over the continuations; after the frame's
//                          barrier the occupancy parts where netocc_backward_kernel forms them, each multiplied by (its own c - Abar_u):
//                          the in-word part of a position 1 from row t - 1 of (alpha, abar), the entry part from E_{t-1}, Ebar_{t-1} and
//                          added to the word's position 0.  One signed double per slot overwrites alpha_t(s).
// The items (frame, mixture, sign * gamma) and their ranking on |gamma| come from the item path (posterior_items.hip).
//
// One workgroup of 512 threads per utterance, slots strided over the threads, FP64, one barrier per frame, no atomics: two identical
// calls return identical bits.  LDS: two rows of (cost, accuracy) = 32 B per position + 384 B for the reduction.  Trellis: rows of
// [alpha[P], abar[P]] = 16 B per (frame, position).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "netfb_device.h"
#include "smbr_device.h"

namespace srgpu {

static constexpr size_t kSmbrLds = 160 * 1024;
static constexpr size_t kSmbrRedBytes = 2 * 3 * kNetFbWaves * 8;  // (m, s, sa) per wave, two parities

// block_lse_read with the third component (smbr_device.h's block_lsea_store)
__device__ inline La block_lsea_read(const double* red) {
  LseA v;
  for (int w = 0; w < kNetFbWaves; w++) v.merge(red[3 * w], red[3 * w + 1], red[3 * w + 2]);
  return v.value();
}

__device__ inline NfCosts smbr_costs(const SmbrArgs& a) {
  const double k = a.scale;
  return NfCosts{k * a.net.tdp_loop, k * a.net.tdp_forward, k * a.net.tdp_skip, k * a.word_penalty, k};
}

// LDS: row[2][2][P] f64 (alpha, abar), red[2][3 * kNetFbWaves] f64
__global__ __launch_bounds__(kNetFbThreads) void smbr_forward_kernel(SmbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  double* al = reinterpret_cast<double*>(smem);
  double* red = al + 4 * (size_t)P;
  double* tr = a.trellis + (f0 - a.group_f0) * 2 * P;  // [T][2][P]
  double* ends = a.ends + (f0 - a.group_f0) * 2;      // [T][2]
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint16_t* ref = a.ref + f0;
  const uint32_t* info = a.net.slot_info;
  const NfCosts c = smbr_costs(a);
  if (T == 0) {
    if (tid == 0) { a.out_cost[u] = kInf; a.out_acc[u] = 0.0; }
    return;
  }
  // the virtual row before frame 0 (parity 1): the start hypothesis at slot 0, cost 0, no frame scored
  for (uint32_t s = tid; s < P; s += kNetFbThreads) {
    al[2 * P + s] = s == 0 ? 0.0 : kInf;
    al[3 * P + s] = 0.0;
  }
  La E{(info[0] & kSlotEnd) ? 0.0 : kInf, 0.0};
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const double* prev = al + (size_t)((t + 1) & 1) * 2 * P;
    const double* preva = prev + P;
    double* cur = al + (size_t)(t & 1) * 2 * P;
    const double* row = row0 + (uint64_t)t * a.ld;
    const uint32_t rf = ref[t];
    LseA we;
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      const double e = c.k * row[f & 0xFFFFu], own = hit(f, rf);
      // the (up to) three sources of the slot, each with the emission it pays and that emission's accuracy: one three-way sum
      const La t0{((f & kSlotEnd) ? kInf : prev[s] + nf_tdp_into(f, 0, c)) + e, preva[s] + own};
      La t1{kInf, 0.0}, t2{kInf, 0.0};
      if (f & kSlotPos0) {
        t1 = La{nf_entry(f, E.x, c) + e, E.a + own};
      } else {
        t1 = La{prev[s - 1] + nf_tdp_into(f, 1, c) + e, preva[s - 1] + own};
        if (f & kSlotPos1) {  // the entry emits the word's first state
          const uint32_t ff = info[s - 1];
          t2 = La{nf_entry(f, E.x, c) + c.k * row[ff & 0xFFFFu], E.a + hit(ff, rf)};
        } else {
          t2 = La{prev[s - 2] + nf_tdp_into(f, 2, c) + e, preva[s - 2] + own};
        }
      }
      La v = la_add3(t0, t1, t2);
      if (!(v.x < kInf)) v = La{kInf, 0.0};
      cur[s] = v.x; cur[P + s] = v.a;
      tr[(size_t)t * 2 * P + s] = v.x; tr[(size_t)t * 2 * P + P + s] = v.a;
      if (f & kSlotEnd) we.add(v.x, v.a);
    }
    block_lsea_store(we, red + (t & 1) * 3 * kNetFbWaves);
    __syncthreads();
    E = block_lsea_read(red + (t & 1) * 3 * kNetFbWaves);
    if (tid == 0) { ends[2 * t] = E.x; ends[2 * t + 1] = E.a; }
  }
  // kappa F_u (the host divides), Abar_u (0 where F_u is not finite: no path, or a -inf emission)
  if (tid == 0) { a.out_cost[u] = E.x; a.out_acc[u] = E.x > -kInf ? E.a : 0.0; }
}

// LDS: row[2][2][P] f64 (beta, bbar), red[2][3 * kNetFbWaves] f64.  Runs after smbr_forward_kernel on the same launch.
__global__ __launch_bounds__(kNetFbThreads) void smbr_backward_kernel(SmbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  double* be = reinterpret_cast<double*>(smem);
  double* red = be + 4 * (size_t)P;
  double* tr = a.trellis + (f0 - a.group_f0) * 2 * P;
  const double* ends = a.ends + (f0 - a.group_f0) * 2;
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint16_t* ref = a.ref + f0;
  const uint32_t* info = a.net.slot_info;
  const NfCosts c = smbr_costs(a);
  const double F = a.out_cost[u], A = a.out_acc[u];  // kappa F_u, Abar_u
  const bool dead = !(F < kInf && F > -kInf);  // no complete path (or a -inf emission took F along): every weight is 0

  for (int t = T - 1; t >= 0; t--) {
    const double* nxt = be + (size_t)((t + 1) & 1) * 2 * P;
    const double* nxta = nxt + P;
    double* cur = be + (size_t)(t & 1) * 2 * P;
    const double* row = row0 + (uint64_t)t * a.ld;
    const double* rn = row + a.ld;  // emissions of the successors (read for t < T - 1 only)
    const bool last = t == T - 1;
    const uint32_t rf = ref[t], rfn = last ? 0xFFFFFFFFu : ref[t + 1];
    La B{kInf, 0.0};
    if (!last) B = block_lsea_read(red + ((t + 1) & 1) * 3 * kNetFbWaves);
    LseA entries;
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      La b;
      if (last) {  // frame T - 1: beta = 0 at the word ends, nothing left to score
        b = La{(f & kSlotEnd) ? 0.0 : kInf, 0.0};
      } else if (f & kSlotEnd) {
        b = B;
      } else {
        const uint32_t f1 = info[s + 1];  // (s is not its word's last position: s + 1 is in the word)
        const La x0{nf_tdp_into(f, 0, c) + c.k * rn[f & 0xFFFFu] + nxt[s], nxta[s] + hit(f, rfn)};
        const La x1{nf_tdp_into(f1, 1, c) + c.k * rn[f1 & 0xFFFFu] + nxt[s + 1], nxta[s + 1] + hit(f1, rfn)};
        const bool two = !(f1 & kSlotEnd);  // s + 2 is in the word too
        const uint32_t s2 = two ? s + 2 : s + 1, f2 = info[s2];
        const La x2{two ? nf_tdp_into(f2, 2, c) + c.k * rn[f2 & 0xFFFFu] + nxt[s2] : kInf, nxta[s2] + hit(f2, rfn)};
        b = la_add3(x0, x1, x2);
      }
      if (!(b.x < kInf)) b = La{kInf, 0.0};
      cur[s] = b.x; cur[P + s] = b.a;
      // the slot's term of B_{t-1}: entry into it at frame t (penalty, the entry's emission at t, beta_t), scored as the first state
      if ((f & (kSlotPos0 | kSlotPos1)) && b.x < kInf) {
        const uint32_t first = (f & kSlotPos0) ? f : info[s - 1];
        entries.add(nf_entry(f, 0.0, c) + c.k * row[first & 0xFFFFu] + b.x, b.a + hit(first, rf));
      }
    }
    block_lsea_store(entries, red + (t & 1) * 3 * kNetFbWaves);
    __syncthreads();
    // (beta_t, bbar_t) is whole in cur: the signed parts over alpha_t in the trellis.  Row t - 1 still holds (alpha, abar).  (Reads
    // cur only; the next frame writes the other row, after its own reads of this one.)
    double* r = tr + (size_t)t * 2 * P;
    const double* ap = r - 2 * P;  // (read for t > 0 only)
    La Ep{(info[0] & kSlotEnd) ? 0.0 : kInf, 0.0};
    if (t > 0) Ep = La{ends[2 * (t - 1)], ends[2 * (t - 1) + 1]};
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      double g = 0.0;
      if (!dead) {
        const double e = c.k * row[f & 0xFFFFu], own = hit(f, rf);
        if (f & kSlotPos1) {  // the in-word part only, term by term (the start hypothesis sits at slot 0, never a position 1)
          const double tail = e + cur[s], rest = own + cur[P + s] - A;
          const double x0 = ((f & kSlotEnd) || t == 0 ? kInf : ap[s] + nf_tdp_into(f, 0, c)) + tail;
          const double x1 = (t > 0 ? ap[s - 1] : (s == 1 ? 0.0 : kInf)) + nf_tdp_into(f, 1, c) + tail;
          if (x0 < kInf) g = exp(F - x0) * (ap[P + s] + rest);
          if (x1 < kInf) g += exp(F - x1) * ((t > 0 ? ap[P + s - 1] : 0.0) + rest);
        } else {
          const double x = r[s] + cur[s];
          if (x < kInf) g = exp(F - x) * (r[P + s] + cur[P + s] - A);
          if ((f & kSlotPos0) && !(f & kSlotEnd)) {  // the entries into position 1 emit this slot's state
            const double y = nf_entry(info[s + 1], Ep.x, c) + e + cur[s + 1];
            if (y < kInf) g += exp(F - y) * (Ep.a + own + cur[P + s + 1] - A);
          }
        }
      }
      r[s] = g;
    }
  }
}

static size_t smbr_smem(uint32_t P) { return (size_t)P * 4 * 8 + kSmbrRedBytes; }
size_t smbr_max_slots() { return (kSmbrLds - kSmbrRedBytes) / 32; }

hipError_t launch_smbr_forward(const SmbrArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  if (a.net.n_slots > smbr_max_slots()) return hipErrorInvalidValue;
  const size_t smem = smbr_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)smbr_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_forward_kernel, dim3(a.n_utts), dim3(kNetFbThreads), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_smbr_backward(const SmbrArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  if (a.net.n_slots > smbr_max_slots()) return hipErrorInvalidValue;
  const size_t smem = smbr_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)smbr_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_backward_kernel, dim3(a.n_utts), dim3(kNetFbThreads), smem, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
