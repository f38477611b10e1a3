// kernels_components.hpp — the connected components of the compacted de Bruijn graph: labels per unitig and per k-mer, sizes per
// component, and the selection of the k-mers of the dropped components for one WordSet::remove_batch. Both forms, as in kernels_gfa.hpp; the input is the
// link table of section 6m (link_start over the 2 U slots, link_to) and the table's `unitig` and `length`.
//   component     a class of the smallest equivalence on the unitigs in which u ~ link_to[l] for every link l of the slots 2 u and 2 u + 1; sides and
//                 link_rev are not looked at
//   par[u]        a unitig of u's component, never above u; between two rounds every par[u] is a root (par[par[u]] == par[u]). par[u] = u at the start, the
//                 smallest unitig of the component in the end
//   a round       hook: nxt = par, then for every link (u, v) with a = par[u] != b = par[v]: nxt[max(a, b)] = min(nxt[max(a, b)], min(a, b)); par is only
//                 read, so the result is the same in every order of the lanes. Compress: pointer jumping on nxt until every entry is a root.
// Plain C++ HIP. The atomics: the min of the hook, the counters that are read back, and the sums of k_cc_sizes (integer adds: order-independent).
#pragma once
#include "kernels_gfa.hpp"

namespace cblx {

// par[u] = u: every unitig a component of its own
__global__ __launch_bounds__(256) void k_cc_init(u64 nu, u32* __restrict__ par) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nu) par[u] = (u32)u;
}

// One lane per slot a (unitig a >> 1): its links against the snapshot `par`. hooked[0] += the slots that issued a hook: a ballot per wave, one LDS sum and
// one atomic per workgroup. hooked is one zeroed word per round.
__global__ __launch_bounds__(256) void k_cc_hook(const u64* __restrict__ link_start, const u32* __restrict__ link_to, const u32* __restrict__ par, u64 nslots,
                                                  u32* __restrict__ nxt, u64* __restrict__ hooked) {
    __shared__ u32 s_cnt[4];
    const u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool hook = false;
    if (a < nslots) {
        const u64 l0 = link_start[a], l1 = link_start[a + 1];
        if (l0 < l1) {
            const u32 pu = par[a >> 1];
            for (u64 l = l0; l < l1; ++l) {
                const u32 v = link_to[l];
                if ((u64)v >= (nslots >> 1)) continue;  // (every link_to is a unitig: no load outside par whatever the table holds)
                const u32 pv = par[v];
                if (pu == pv) continue;
                atomicMin(nxt + (pu > pv ? pu : pv), pu > pv ? pv : pu);
                hook = true;
            }
        }
    }
    const u32 w = (u32)__builtin_popcountll(__ballot(hook));
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t) atomicAdd((unsigned long long*)hooked, (unsigned long long)t);
    }
}

// One jump, from p into p2, never in place: p2[u] = p[p[u]]. open[0] += the unitigs that were neither a root nor the child of one when the launch began
// (0: p was compressed, and p2 == p). open is one zeroed word per launch.
__global__ __launch_bounds__(256) void k_cc_jump(const u32* __restrict__ p, u64 nu, u32* __restrict__ p2, u64* __restrict__ open) {
    __shared__ u32 s_cnt[4];
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool far = false;
    if (u < nu) {
        const u32 a = p[u], g = p[a];
        p2[u] = g;
        far = g != a;
    }
    const u32 w = (u32)__builtin_popcountll(__ballot(far));
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t) atomicAdd((unsigned long long*)open, (unsigned long long)t);
    }
}

// root[u] = 1 where u is the smallest unitig of its component: the input of the scan that numbers the components by ascending `first`
__global__ __launch_bounds__(256) void k_cc_roots(const u32* __restrict__ par, u64 nu, u32* __restrict__ root) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nu) root[u] = par[u] == (u32)u ? 1u : 0u;
}
// component[u] = scan[par[u]] (scan: the exclusive scan of k_cc_roots), and a root writes first[component] = u
__global__ __launch_bounds__(256) void k_cc_number(const u32* __restrict__ par, const u32* __restrict__ scan, u64 nu, u32* __restrict__ component, u32* __restrict__ first) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nu) return;
    const u32 r = par[u], c = scan[r];
    component[u] = c;
    if (r == (u32)u) first[c] = (u32)u;
}

// One lane per unitig: unitigs[c] += 1 and kmers[c] += length[u] (both zeroed by the caller). One giant component would put every lane on one address, so
// the lanes whose component is that of the wave's first active lane are summed in the wave and that lane issues one pair of atomics; the others issue their own.
__global__ __launch_bounds__(256) void k_cc_sizes(const u32* __restrict__ component, const u32* __restrict__ length, u64 nu, u32* __restrict__ unitigs,
                                                   u64* __restrict__ kmers) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = u < nu;
    const u32 c = active ? component[u] : 0u, len = active ? length[u] : 0u;
    const u64 live = __ballot(active);
    if (live == 0) return;  // wave-uniform
    const u32 lead = (u32)__builtin_ctzll(live);
    const u32 c0 = (u32)__shfl((int)c, (int)lead, 64);
    const bool same = active && c == c0;
    const u32 cnt = (u32)__builtin_popcountll(__ballot(same));
    const u64 sum = wave_reduce_sum<u64>(same ? (u64)len : 0ull);
    if (!active) return;
    if (same) {
        if (lane_id() != lead) return;
        atomicAdd(unitigs + c0, cnt);
        atomicAdd((unsigned long long*)(kmers + c0), (unsigned long long)sum);
    } else {
        atomicAdd(unitigs + c, 1u);
        atomicAdd((unsigned long long*)(kmers + c), (unsigned long long)len);
    }
}

// One lane per stored k-mer: the component of its unitig
__global__ __launch_bounds__(256) void k_cc_kmer(const u32* __restrict__ unitig, const u32* __restrict__ component, u64 n, u32* __restrict__ kmer_component) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kmer_component[i] = component[unitig[i]];
}

// One lane per component: keep[c] = 1 where the filter leaves it — `only` != ~0: the one component `only`; otherwise those of at least min_kmers k-mers
__global__ __launch_bounds__(256) void k_cc_keep(const u64* __restrict__ kmers, u64 nc, u64 min_kmers, u32 only, u8* __restrict__ keep) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nc) keep[c] = only != 0xFFFFFFFFu ? (u8)((u32)c == only) : (u8)(kmers[c] >= min_kmers);
}
// One lane per stored k-mer: sel[i] = 1 when its component is dropped, the input of the scan that gives the output positions
__global__ __launch_bounds__(256) void k_cc_select(const u32* __restrict__ unitig, const u32* __restrict__ component, const u8* __restrict__ keep, u64 n,
                                                    u32* __restrict__ sel) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sel[i] = keep[component[unitig[i]]] == 0 ? 1u : 0u;
}
// One export pass: k-mer i of the pass has ordinal e0 + i; a selected one stores its packed k-mer at pos[e0 + i], the exclusive scan of sel, so the output
// is in iteration order. out_hi is null for K <= 31 (and k_hi with it).
__global__ __launch_bounds__(256) void k_cc_gather(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ sel,
                                                    const u32* __restrict__ pos, u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || sel[e0 + i] == 0) return;
    const u32 p = pos[e0 + i];
    out_lo[p] = k_lo[i];
    if (out_hi) out_hi[p] = k_hi ? k_hi[i] : 0ull;
}

}  // namespace cblx
