// pdl_split.h — K-split: the first level of Girvan-Newman on a batch of ordered graphs (pdl_split_first_level; included at the
// end of pdl_bbh.hip).  What netclu.girvan_newman_first_level does to a component that holds a collision: Brandes' edge
// betweenness of the whole graph, the first edge of the edge list with the largest value removed, again, until the removed
// edge's two ends are no longer connected.  The ORDERS — of the nodes, of every node's neighbours, of the edge list — are the
// host's (netclu.py follows networkx's dicts and sets); they arrive flattened and stay as they are: a removal is a mark on the
// edge's two slots.  The arithmetic is the device's, and it is the Python's operation for operation:
//
//   * doubles throughout, and no fused multiply-add: `sigma[v] * coeff` is rounded before it is added (the pragma in the kernel;
//     -O3 would contract it);
//   * one LANE walks one source serially — the queue of the breadth-first search, `sigma[w] += sigma[v]` and, popping the order
//     from the back, `coeff = (1 + delta[w]) / sigma[w]`, `delta[v] += sigma[v] * coeff` come in the order the Python has them.
//     (A node's predecessors are found again as the neighbours one level nearer: the Python walks them in the order they were
//     dequeued, here they come in neighbour order — every predecessor feeds its own delta and its own edge, so no sum sees the
//     difference);
//   * an edge's betweenness takes its contributions IN SOURCE ORDER: the lanes of a workgroup take SPLIT_L sources at a time and
//     leave each source's contribution per edge in contrib[lane][edge] (an edge lies on the shortest-path graph of a source in one
//     direction at most: one store; 0.0 where it does not, and x + 0.0 = x for the x >= 0 here); then a lane per edge adds the
//     SPLIT_L values onto bet[edge] one by one, and clears them.  Chunk follows chunk;
//   * `bet *= 1 / (n (n - 1))` is done (it can make ties), the arg-max is on (value, lowest edge index).
//
// One workgroup owns one graph and loops over the removals by itself: no host round trip per removal, nothing waits for
// another workgroup, and every loop has its bound before it starts (at most m removals, n sources, n queue entries, n levels).
// The adjacency (offsets, neighbours with the removed marks, edge ids of the slots) sits in LDS where it fits, else the marks are
// in the workgroup's scratch.  Per-lane state and contrib live in the workgroup's slice of an HBM scratch the host sizes; a batch
// is cut into launches under option "split_scratch_bytes".
//
// Everything the kernel indexes with is checked on the host first (split_prepare): offsets, neighbour indices, self loops,
// repeats, one-directional edges -> PDL_ERR_ARGUMENT before anything is uploaded.
#pragma once

#include "pdl_common.h"

#include <algorithm>

constexpr uint32_t SPLIT_L = 256;              // lanes of a workgroup = sources of a chunk
constexpr uint32_t SPLIT_LDS_WORDS = 12288;    // 48 KB of adjacency in LDS
constexpr uint32_t SPLIT_GONE = 0xffffffffu;   // a removed slot

struct SplitDesc {
    uint32_t node0, n;        // first node (row of adj_off), nodes
    uint32_t slot0, S;        // first adjacency slot, slots (2 m)
    uint32_t edge0, m;        // first edge (row of ends / slots / out_edge), edges
    uint64_t scratch;         // byte offset of the workgroup's slice
};
// bytes of scratch of a graph: bet [m] | contrib [L][m] | sigma, delta [n][L] (doubles) | dist, order [n][L] | mark [n] | wadj [S]
static inline uint64_t split_scratch_bytes(uint64_t n, uint64_t m) {
    if (m == 0) return 0;
    const uint64_t b = 8 * (m + SPLIT_L * m + 2 * SPLIT_L * n) + 4 * (2 * SPLIT_L * n + n + 2 * m);
    return (b + 255) & ~255ull;
}

__device__ __forceinline__ void split_sync() { __threadfence_block(); pdl_sync(); __threadfence_block(); }     // (the scratch in HBM changes hands between the lanes)

__global__ __launch_bounds__(256) void k_split(const SplitDesc *desc, const uint32_t *adj_off, const uint32_t *adj, const uint32_t *eid_g, const uint2 *ends,
                                               const uint2 *slots, uint8_t *scratch, uint32_t *out_edge, uint32_t *out_count) {
    // No fused multiply-add.  The pragma holds for THIS function body only: all of the betweenness arithmetic stays in it — a
    // helper factored out of it would need the pragma of its own, or -O3 contracts its `a * b + c` again.
#pragma clang fp contract(off)
    __shared__ uint32_t s_mem[SPLIT_LDS_WORDS];
    __shared__ double s_val[256];
    __shared__ uint32_t s_idx[256];
    __shared__ uint32_t s_flag;
    const SplitDesc d = desc[blockIdx.x];
    const uint32_t t = threadIdx.x, n = d.n, m = d.m, S = d.S;
    if (m == 0) { if (t == 0) out_count[blockIdx.x] = 0; return; }
    uint8_t *sp = scratch + d.scratch;
    double *bet = reinterpret_cast<double *>(sp); sp += 8ull * m;
    double *contrib = reinterpret_cast<double *>(sp); sp += 8ull * SPLIT_L * m;
    double *sigma = reinterpret_cast<double *>(sp); sp += 8ull * SPLIT_L * n;
    double *delta = reinterpret_cast<double *>(sp); sp += 8ull * SPLIT_L * n;
    int32_t *dist = reinterpret_cast<int32_t *>(sp); sp += 4ull * SPLIT_L * n;
    uint32_t *order = reinterpret_cast<uint32_t *>(sp); sp += 4ull * SPLIT_L * n;
    int32_t *mark = reinterpret_cast<int32_t *>(sp); sp += 4ull * n;
    const bool in_lds = (uint64_t) n + 1 + 2ull * S <= SPLIT_LDS_WORDS;
    const uint32_t *off, *eid;        // off[v] - base .. off[v + 1] - base: the slots of node v
    uint32_t *wadj, base;
    if (in_lds) {
        for (uint32_t i = t; i <= n; i += 256) s_mem[i] = adj_off[d.node0 + i] - d.slot0;
        for (uint32_t k = t; k < S; k += 256) { s_mem[n + 1 + k] = adj[d.slot0 + k]; s_mem[n + 1 + S + k] = eid_g[d.slot0 + k]; }
        off = s_mem; wadj = s_mem + n + 1; eid = s_mem + n + 1 + S; base = 0;
    } else {
        wadj = reinterpret_cast<uint32_t *>(sp);
        for (uint32_t k = t; k < S; k += 256) wadj[k] = adj[d.slot0 + k];
        off = adj_off + d.node0; eid = eid_g + d.slot0; base = d.slot0;
    }
    for (uint32_t e = t; e < m; e += 256) bet[e] = 0.0;
    for (uint64_t i = t; i < (uint64_t) SPLIT_L * m; i += 256) contrib[i] = 0.0;
    split_sync();

    const double scale = 1.0 / (double) ((uint64_t) n * (n - 1));
    uint32_t removed = 0;
    for (uint32_t round = 0; round < m; round++) {
        for (uint32_t c0 = 0; c0 < n; c0 += SPLIT_L) {
            const uint32_t s = c0 + t;
            if (s < n) {
#define AT(i) ((size_t) (i) * SPLIT_L + t)
                for (uint32_t i = 0; i < n; i++) dist[AT(i)] = -1;
                dist[AT(s)] = 0; sigma[AT(s)] = 1.0; delta[AT(s)] = 0.0; order[AT(0)] = s;
                uint32_t head = 0, tail = 1;          // (tail <= n: a node is queued once, when its distance is set)
                while (head < tail) {
                    const uint32_t v = order[AT(head)]; head++;
                    const int32_t dv = dist[AT(v)];
                    const double sv = sigma[AT(v)];
                    const uint32_t k1 = off[v + 1] - base;
                    for (uint32_t k = off[v] - base; k < k1; k++) {
                        const uint32_t w = wadj[k];
                        if (w == SPLIT_GONE) continue;
                        const int32_t dw = dist[AT(w)];
                        if (dw < 0) { order[AT(tail)] = w; tail++; dist[AT(w)] = dv + 1; sigma[AT(w)] = sv; delta[AT(w)] = 0.0; }     // (0.0 + sv)
                        else if (dw == dv + 1) sigma[AT(w)] = sigma[AT(w)] + sv;
                    }
                }
                double *mine = contrib + (size_t) t * m;
                for (uint32_t q = tail; q-- > 0;) {
                    const uint32_t w = order[AT(q)];
                    const int32_t dw = dist[AT(w)];
                    const double coeff = (1.0 + delta[AT(w)]) / sigma[AT(w)];
                    const uint32_t k1 = off[w + 1] - base;
                    for (uint32_t k = off[w] - base; k < k1; k++) {
                        const uint32_t v = wadj[k];
                        if (v == SPLIT_GONE || dist[AT(v)] + 1 != dw) continue;
                        const double c = sigma[AT(v)] * coeff;
                        mine[eid[k]] = c;
                        delta[AT(v)] = delta[AT(v)] + c;
                    }
                }
#undef AT
            }
            split_sync();
            const uint32_t cnt = n - c0 < SPLIT_L ? n - c0 : SPLIT_L;
            for (uint32_t e = t; e < m; e += 256) {
                double b = bet[e];
                for (uint32_t l = 0; l < cnt; l++) { const size_t at = (size_t) l * m + e; b = b + contrib[at]; contrib[at] = 0.0; }
                bet[e] = b;
            }
            split_sync();
        }
        // the first edge with the largest scaled value
        double best = -1.0;
        uint32_t bi = SPLIT_GONE;
        for (uint32_t e = t; e < m; e += 256) {
            const double b = bet[e] * scale;
            bet[e] = 0.0;
            if (wadj[slots[d.edge0 + e].x - d.slot0] != SPLIT_GONE && b > best) { best = b; bi = e; }
        }
        s_val[t] = best; s_idx[t] = bi;
        split_sync();
        for (uint32_t stride = 128; stride; stride >>= 1) {
            if (t < stride) {
                const double ov = s_val[t + stride]; const uint32_t oi = s_idx[t + stride];
                if (ov > s_val[t] || (ov == s_val[t] && oi < s_idx[t])) { s_val[t] = ov; s_idx[t] = oi; }
            }
            split_sync();
        }
        const uint32_t e = s_idx[0];
        if (e >= m) break;                       // (no live edge: cannot be, the last removal ended the loop)
        const uint2 uv = ends[d.edge0 + e];
        if (t == 0) {
            out_edge[d.edge0 + removed] = e;
            const uint2 sl = slots[d.edge0 + e];
            wadj[sl.x - d.slot0] = SPLIT_GONE; wadj[sl.y - d.slot0] = SPLIT_GONE;
        }
        removed++;
        // is uv.y still reachable from uv.x?  Level by level, the whole workgroup (lanes that meet at a node store the same level
        // and the same flag: whoever wins, the level's outcome is one)
        for (uint32_t i = t; i < n; i += 256) mark[i] = i == uv.x ? 0 : -1;
        split_sync();
        bool connected = false;
        for (uint32_t level = 0; level < n; level++) {
            if (t == 0) s_flag = 0;
            split_sync();
            for (uint32_t i = t; i < n; i += 256) {
                if (mark[i] != (int32_t) level) continue;
                const uint32_t k1 = off[i + 1] - base;
                for (uint32_t k = off[i] - base; k < k1; k++) {
                    const uint32_t w = wadj[k];
                    if (w != SPLIT_GONE && mark[w] < 0) { mark[w] = (int32_t) level + 1; s_flag = 1; }
                }
            }
            split_sync();
            const uint32_t grew = s_flag;
            const int32_t mv = mark[uv.y];
            split_sync();
            if (mv >= 0) { connected = true; break; }
            if (!grew) break;
        }
        if (!connected) break;
    }
    if (t == 0) out_count[blockIdx.x] = removed;
}

// What the host makes of a packed batch before anything goes to the device: every check of the contract, the edge list of every
// graph (edge ids in `G.edges()` order: the slots that point to a later node, in slot order), the edge id of every slot, both
// slots of every edge.
struct SplitPrep {
    std::vector<SplitDesc> desc;
    std::vector<uint32_t> adj_off, eid;       // [nodes + 1] (32-bit), [slots]
    std::vector<uint2> ends, slots;           // [edges] (u, v) local; (slot of u -> v, slot of v -> u) global
};
static void split_prepare(uint32_t n_graphs, const uint64_t *node_off, const uint64_t *adj_off, const uint32_t *adj, SplitPrep &p) {
    const char *who = "pdl_split_first_level";
    if (node_off[0] != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: node_off[0] = %llu, not 0", who, (unsigned long long) node_off[0]);
    for (uint32_t j = 0; j < n_graphs; j++)
        if (node_off[j + 1] < node_off[j]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: node_off decreases at graph %u", who, j);
    const uint64_t nodes = node_off[n_graphs];
    if (nodes >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s: 2^31 nodes and more", who);
    if (adj_off[0] != 0) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: adj_off[0] = %llu, not 0", who, (unsigned long long) adj_off[0]);
    for (uint64_t i = 0; i < nodes; i++)
        if (adj_off[i + 1] < adj_off[i]) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: adj_off decreases at node %llu", who, (unsigned long long) i);
    const uint64_t total = adj_off[nodes];
    if (total >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%s: 2^31 adjacency slots and more", who);
    if (total && !adj) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: NULL pointer", who);
    p.desc.assign(n_graphs, SplitDesc{});
    p.adj_off.resize(nodes + 1);
    for (uint64_t i = 0; i <= nodes; i++) p.adj_off[i] = (uint32_t) adj_off[i];
    p.eid.assign(total, 0);
    p.ends.clear(); p.slots.clear();
    std::vector<uint64_t> seen;                                 // [local node] 1 + the global node that named it last
    std::vector<std::pair<uint64_t, uint32_t>> fwd;             // (u << 32 | v, edge id) of the graph's forward slots
    for (uint32_t j = 0; j < n_graphs; j++) {
        const uint64_t a = node_off[j], n = node_off[j + 1] - a;
        SplitDesc &d = p.desc[j];
        d.node0 = (uint32_t) a; d.n = (uint32_t) n; d.slot0 = (uint32_t) adj_off[a]; d.S = (uint32_t) (adj_off[a + n] - adj_off[a]);
        d.edge0 = (uint32_t) p.ends.size();
        seen.assign(n, 0);
        fwd.clear();
        uint64_t backward = 0;
        for (uint64_t u = 0; u < n; u++)
            for (uint64_t k = adj_off[a + u]; k < adj_off[a + u + 1]; k++) {
                const uint64_t v = adj[k];
                if (v >= n) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: graph %u, node %llu names neighbour %llu of %llu nodes", who, j, (unsigned long long) u, (unsigned long long) v, (unsigned long long) n);
                if (v == u) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: graph %u, node %llu is its own neighbour", who, j, (unsigned long long) u);
                if (seen[v] == a + u + 1) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: graph %u, node %llu names neighbour %llu twice", who, j, (unsigned long long) u, (unsigned long long) v);
                seen[v] = a + u + 1;
                if (v > u) {
                    const uint32_t e = (uint32_t) fwd.size();
                    fwd.push_back({u << 32 | v, e});
                    p.eid[k] = e;
                    p.ends.push_back(make_uint2((uint32_t) u, (uint32_t) v));
                    p.slots.push_back(make_uint2((uint32_t) k, SPLIT_GONE));
                } else backward++;
            }
        if (backward != fwd.size()) PDL_FAIL(PDL_ERR_ARGUMENT, "%s: graph %u holds an edge in one direction only", who, j);
        d.m = (uint32_t) fwd.size();
        std::sort(fwd.begin(), fwd.end());
        for (uint64_t u = 0; u < n; u++)
            for (uint64_t k = adj_off[a + u]; k < adj_off[a + u + 1]; k++) {
                const uint64_t v = adj[k];
                if (v > u) continue;
                const auto it = std::lower_bound(fwd.begin(), fwd.end(), std::make_pair(v << 32 | u, 0u));
                if (it == fwd.end() || it->first != (v << 32 | u))
                    PDL_FAIL(PDL_ERR_ARGUMENT, "%s: graph %u, edge %llu -> %llu is there in one direction only", who, j, (unsigned long long) u, (unsigned long long) v);
                p.eid[k] = it->second;
                p.slots[d.edge0 + it->second].y = (uint32_t) k;
            }
    }
}

void pdl_run_split(pdl_ctx *c, uint32_t n_graphs, const uint64_t *node_off, const uint64_t *adj_off, const uint32_t *adj, pdl_split_result &out) {
    hipStream_t st = c->stream;
    out = pdl_split_result{};
    SplitPrep p;
    split_prepare(n_graphs, node_off, adj_off, adj, p);
    // the chunks: graphs in order, as many as fit the budget
    const uint64_t budget = c->opt_split_scratch_bytes;
    std::vector<uint32_t> chunk_begin{0};
    uint64_t used = 0, most = 0;
    for (uint32_t j = 0; j < n_graphs; j++) {
        const uint64_t need = split_scratch_bytes(p.desc[j].n, p.desc[j].m);
        if (need > budget)
            PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_split_first_level: graph %u (%u nodes, %u edges) needs %llu bytes of scratch, split_scratch_bytes is %llu", j,
                     p.desc[j].n, p.desc[j].m, (unsigned long long) need, (unsigned long long) budget);
        if (used + need > budget) { chunk_begin.push_back(j); used = 0; }
        p.desc[j].scratch = used;
        used += need;
        most = std::max(most, used);
    }
    chunk_begin.push_back(n_graphs);
    const uint64_t nodes = node_off[n_graphs], total = adj_off[nodes], edges = p.ends.size();
    out.graphs = n_graphs; out.nodes = nodes; out.edges = edges;
    out.removed_off.assign((size_t) n_graphs + 1, 0);
    if (edges == 0) return;
    pdl_ctx::SplitBufs &b = c->sb;
    b.desc.alloc(n_graphs * sizeof(SplitDesc)); b.adj_off.alloc((nodes + 1) * 4); b.adj.alloc(total * 4); b.eid.alloc(total * 4);
    b.ends.alloc(edges * 8); b.slots.alloc(edges * 8); b.out_edge.alloc(edges * 4); b.out_count.alloc((size_t) n_graphs * 4); b.scratch.alloc(most);
    PDL_HIP(hipMemcpyAsync(b.desc.p, p.desc.data(), n_graphs * sizeof(SplitDesc), hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(b.adj_off.p, p.adj_off.data(), (nodes + 1) * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(b.adj.p, adj, total * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(b.eid.p, p.eid.data(), total * 4, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(b.ends.p, p.ends.data(), edges * 8, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(b.slots.p, p.slots.data(), edges * 8, hipMemcpyHostToDevice, st));
    b.spans.start(st);
    b.spans.begin();
    for (size_t ch = 0; ch + 1 < chunk_begin.size(); ch++) {          // (one stream: a chunk has the scratch to itself)
        const uint32_t j0 = chunk_begin[ch], cnt = chunk_begin[ch + 1] - j0;
        hipLaunchKernelGGL(k_split, dim3(cnt), dim3(256), 0, st, b.desc.as<SplitDesc>() + j0, b.adj_off.as<uint32_t>(), b.adj.as<uint32_t>(), b.eid.as<uint32_t>(),
                           b.ends.as<uint2>(), b.slots.as<uint2>(), b.scratch.as<uint8_t>(), b.out_edge.as<uint32_t>(), b.out_count.as<uint32_t>() + j0);
        PDL_HIP(hipGetLastError());
        out.chunks++;
    }
    b.spans.end();
    std::vector<uint32_t> h_count, h_edge;
    copy_down(st, h_count, b.out_count.p, n_graphs); copy_down(st, h_edge, b.out_edge.p, edges);
    PDL_HIP(hipStreamSynchronize(st));
    out.device_ms = b.spans.total_ms();
    for (uint32_t j = 0; j < n_graphs; j++) {
        const SplitDesc &d = p.desc[j];
        if (h_count[j] > d.m) PDL_FAIL(PDL_ERR_DEVICE, "K-split: graph %u reports %u removals of %u edges", j, h_count[j], d.m);
        for (uint32_t r = 0; r < h_count[j]; r++) {
            const uint32_t e = h_edge[d.edge0 + r];
            if (e >= d.m) PDL_FAIL(PDL_ERR_DEVICE, "K-split: graph %u removed edge %u of %u", j, e, d.m);
            out.removed_u.push_back(p.ends[d.edge0 + e].x); out.removed_v.push_back(p.ends[d.edge0 + e].y);
        }
        out.removed_off[j + 1] = out.removed_u.size();
    }
    out.rounds = out.removed_u.size();
}
