// Density clustering (DBSCAN) inside each cloud of a ragged batch, and the filter that drops small clusters.  The
// definition is in include/rald_hip.h; in short, with the layout, the box, d2 and r2 = fl(eps * eps) of radius_search.hip
//   count[i]  the inside rows j != i of the same cloud with d2(i,j) <= r2, capped at min_points; -1 outside
//   core      an inside row with count >= min_points (min_points = 0: every inside row)
//   cluster   a connected component of the core rows under d2 <= r2, numbered by its smallest row index in ascending order
//   border    an inside row that is not core: the cluster of its nearest core row within r2, the smallest row index on equal d2
//   labels    the cluster, -1 for noise, -2 outside the box; sizes count core and border rows
//   filter    keep row i iff label >= 0 and sizes[label] >= min_cluster_size (and, with largest_only, label = the argmax of the sizes)
// Launches behind the index (cloud_index.hip), all on one stream:
//   clu_init      (256 rows, cloud)              parent[i] = i
//   clu_count     (256 sorted positions, cloud)  the walk of rad_count with cap = min_points; the core flag in SORTED order beside the
//                                                count by row.  Skipped for min_points = 0
//   clu_link      (256 sorted positions, cloud)  the same walk: a core lane unites itself with every core neighbour of SMALLER row
//                                                index (each edge once); any other inside lane notes its nearest core neighbour
//   clu_flatten   (1024 rows, cloud)             every row's root (a border row: its nearest core row's), the count of core roots per block
//   cloud_block_scan, cloud_offsets              the scans of the compaction: the rank of a core root is its cluster id, the total C
//   clu_number    (1024 rows, cloud)             a core root's cluster id to its row; sizes = 0
//   clu_label     (256 rows, cloud)              labels, sizes (one integer atomicAdd per wave and label), num_clusters
// and for the filter clu_argmax (cloud), clu_keep (256 rows, cloud), the compaction of cloud_index.hip and its cloud_kept_labels.
// The union-find keeps ONE invariant: parent[x] <= x, and parent[x] is in x's tree.  A union hooks the LARGER root under the smaller
// with a device-scope compare-and-swap and, when that fails, finds both roots again: a root only ever moves down, so the final root
// of a component is its smallest row whatever the order of arrival.  Path halving writes with atomicMin a value read from the chain.
// Inside clu_link every read of parent is a relaxed device-scope atomic load (the XCDs' L2s are not coherent for plain loads); the
// kernels behind it may use plain loads.  Every loop is bounded by the cloud's length (<= max_per_sample, a host value), by the
// grid's dims or by 32; a lane that exhausts a bound stops.  A row index read from the scratch is clamped into the cloud before it
// addresses anything.  clu_count and clu_link walk with radius_walk of cloud_index.h, as rad_count does.
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int CLU_T = 256;                                   // rows or sorted positions per workgroup of the per-row kernels

struct ClusterArgs {
    RaggedCloud c;
    CellGrid g;
    float r2, rs;
    int min_points, min_size, largest;
    const unsigned* skey; const float4* srow;                // [n_total] the sorted keys and rows
    unsigned char* score;                                    // [n_total] per SORTED position: the row is core (min_points > 0)
    int32_t* cnt;                                            // [n_total] per row
    int* parent;                                             // [n_total] per row, an index inside the cloud
    int* aux;                                                // [n_total] per row.  clu_link: the row itself (core), its nearest core row
                                                             // (border), -1 (noise), -2 (outside); clu_number: a core root's cluster id
    int* root;                                               // [n_total] per row.  clu_flatten: the root, -1, -2; clu_keep: the keep flag
    int32_t* labels; int32_t* sizes; int32_t* nclu;          // the outputs of the labels call, or scratch
    int* best;                                               // [batch] the largest cluster
    int64_t* kept;                                           // [n_total] the kept rows' indices (out_index, or scratch)
    BlockScan num, sc;                                       // the numbering of the core roots, the filter's compaction
};

__global__ __launch_bounds__(CLU_T) void clu_init(ClusterArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLU_T + threadIdx.x;
    if (j >= n) return;
    a.parent[row0 + j] = (int)j;
}

__global__ __launch_bounds__(CLU_T) void clu_count(ClusterArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLU_T + threadIdx.x;
    if (j >= n) return;
    const unsigned* sk = a.skey + row0;
    const float4* sr = a.srow + row0;
    const float4 me = sr[j];
    const int i = rad_clamp(__float_as_int(me.w), n);
    int count = -1;
    if (sk[j] < a.g.cells) {
        count = 0;
        const float r2 = a.r2;
        const int cap = a.min_points;
        radius_walk(a.g, a.rs, sk, sr, n, me,[&](int, const float4& o, float d2) {
            if (__float_as_int(o.w) != i && d2 <= r2) return ++count == cap;
            return false;
        });
    }
    a.cnt[row0 + i] = count;
    a.score[row0 + j] = count >= a.min_points;
}

__device__ __forceinline__ int clu_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as this lane sees it; every step descends strictly, so at most n of them
__device__ __forceinline__ int clu_find(int* p, int x, int n) {
    for (int s = 0; s < n; ++s) {
        const int px = rad_clamp(clu_load(p + x), n);
        if (px >= x) break;                                  // a root
        const int gp = rad_clamp(clu_load(p + px), n);
        if (gp >= px) return px;
        atomicMin(p + x, gp);                                // path halving: gp is in x's tree and below x
        x = gp;
    }
    return x;
}

// joins the trees of x and y -> the joint root as this lane sees it.  A failed compare-and-swap means that root moved down: at most n
// retries
__device__ __forceinline__ int clu_unite(int* p, int x, int y, int n) {
    for (int t = 0; t < n; ++t) {
        x = clu_find(p, x, n);
        y = clu_find(p, y, n);
        if (x == y) return x;
        const int hi = x > y ? x : y, lo = x > y ? y : x;
        if (atomicCAS(p + hi, hi, lo) == hi) return lo;
    }
    return x;
}

__global__ __launch_bounds__(CLU_T) void clu_link(ClusterArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLU_T + threadIdx.x;
    if (j >= n) return;
    const unsigned* sk = a.skey + row0;
    const float4* sr = a.srow + row0;
    const unsigned char* core = a.score + row0;
    const bool all = a.min_points == 0;                      // every inside row is core
    int* parent = a.parent + row0;
    const float4 me = sr[j];
    const int i = rad_clamp(__float_as_int(me.w), n);
    const bool inside = sk[j] < a.g.cells;
    int state = -2;
    if (inside) {
        const bool mine = all || core[j];
        const float r2 = a.r2;
        int bestj = -1, top = i;                             // top: a row of i's tree, its root when this lane last saw it
        float best = INFINITY;
        radius_walk(a.g, a.rs, sk, sr, n, me,[&](int q, const float4& o, float d2) {
            const int jr = rad_clamp(__float_as_int(o.w), n);
            if (jr != i && d2 <= r2 && (all || core[q])) {
                if (mine) {
                    // a neighbour whose parent is `top` is in i's tree already: seen without a read of the root, which in a large
                    // component is the one address that every lane would read at every edge
                    if (jr < i && rad_clamp(clu_load(parent + jr), n) != top) top = clu_unite(parent, top, jr, n);
                } else if (d2 < best || (d2 == best && jr < bestj)) {
                    best = d2; bestj = jr;
                }
            }
            return false;
        });
        state = mine ? i : bestj;
    }
    a.aux[row0 + i] = state;
    if (all) a.cnt[row0 + i] = inside ? 0 : -1;
}

__device__ __forceinline__ bool clu_is_root(const ClusterArgs& a, int64_t row0, int64_t j, int n) {
    return j < n && a.aux[row0 + j] == (int)j && a.root[row0 + j] == (int)j;
}

__global__ __launch_bounds__(CLOUD_SEG) void clu_flatten(ClusterArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;        // the whole workgroup
    bool flag = false;
    if (j < n) {
        int r = a.aux[row0 + j];
        if (r >= 0) {
            const int* parent = a.parent + row0;
            r = rad_clamp(r, n);
            for (int s = 0; s < n; ++s) {
                const int pr = rad_clamp(parent[r], n);
                if (pr >= r) break;
                r = pr;
            }
            flag = a.aux[row0 + j] == (int)j && r == (int)j;
        }
        a.root[row0 + j] = r;
    }
    int total;
    block_rank<CLOUD_SEG>(flag, sh, tid, &total);
    if (tid == 0) a.num.blocks[(int64_t)b * a.num.nseg_max + blockIdx.x] = total;
}

__global__ __launch_bounds__(CLOUD_SEG) void clu_number(ClusterArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    if ((int64_t)blockIdx.x * CLOUD_SEG >= n) return;
    const bool flag = clu_is_root(a, row0, j, n);
    const int in_block = block_rank<CLOUD_SEG>(flag, sh, tid, nullptr);
    if (j >= n) return;                                      // no barrier below
    a.sizes[row0 + j] = 0;
    if (flag) a.aux[row0 + j] = a.num.blocks[(int64_t)b * a.num.nseg_max + blockIdx.x] + in_block;
}

__global__ __launch_bounds__(CLU_T) void clu_label(ClusterArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.nclu[b] = a.num.total[b];
    const int64_t j = (int64_t)blockIdx.x * CLU_T + threadIdx.x;
    if (j >= n) return;
    int label = a.root[row0 + j];
    if (label >= 0) label = rad_clamp(a.aux[row0 + rad_clamp(label, n)], n);
    a.labels[row0 + j] = label;
    // one add per wave and label, not per row: a cluster of most of the cloud would otherwise take every row's add at one address
    const bool counted = label >= 0;                         // core and border rows
    unsigned long long todo = __ballot(counted);
    for (int it = 0; it < 64 && todo; ++it) {
        const int first = __builtin_amdgcn_readlane(label, __builtin_ctzll(todo));
        const unsigned long long same = __ballot(counted && label == first);
        if (counted && label == first && (int)(threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(a.sizes + row0 + first, __popcll(same));
        todo &= ~same;
    }
}

// the cluster of the largest size, the smallest id on equal sizes; -1 without a cluster
__global__ __launch_bounds__(CLU_T) void clu_argmax(ClusterArgs a) {
    __shared__ int sv[CLU_T], sc[CLU_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    int C = a.nclu[b];
    C = C < n ? C : n;
    int bv = 0, bc = -1;
    for (int c = tid; c < C; c += CLU_T) {                   // ascending ids: a later one wins only when larger
        const int v = a.sizes[row0 + c];
        if (v > bv) { bv = v; bc = c; }
    }
    block_argmax<CLU_T>(bv, bc, sv, sc, tid);
    if (tid == 0) a.best[b] = sc[0];
}

__global__ __launch_bounds__(CLU_T) void clu_keep(ClusterArgs a) {
    const int b = blockIdx.y;
    int64_t row0;
    const int n = ragged_span(a.c, b, row0);
    const int64_t j = (int64_t)blockIdx.x * CLU_T + threadIdx.x;
    if (j >= n) return;
    const int label = a.labels[row0 + j];
    bool keep = label >= 0;
    if (keep) keep = a.sizes[row0 + rad_clamp(label, n)] >= a.min_size && (!a.largest || label == a.best[b]);
    a.root[row0 + j] = keep;
}

void clu_layout(ClusterArgs& a, CloudIndex& ix, Carver& s, int64_t chunk) {
    const int64_t T = a.c.n_total;
    cloud_index_layout(ix, a.c, s, chunk, true);
    a.cnt = s.take<int32_t>(T);
    a.score = s.take<unsigned char>(T);
    a.parent = s.take<int>(T);
    a.aux = s.take<int>(T);
    a.root = s.take<int>(T);
    a.labels = s.take<int32_t>(T);
    a.sizes = s.take<int32_t>(T);
    a.kept = s.take<int64_t>(T);
    a.nclu = s.take<int32_t>(a.c.batch);
    a.best = s.take<int>(a.c.batch);
    block_scan_layout(a.num, a.c, s);
    a.num.out_offsets = s.take<int64_t>(a.c.batch + 1);
    block_scan_layout(a.sc, a.c, s);
}

// the checks of both entries in the radius entries' order, then the index and the launches up to the labels
int clu_labels(const std::string& who, ClusterArgs& a, const RaggedCloud& c, const GridSpec& grid, float eps, int min_points,
               int32_t* out_labels, int32_t* out_num_clusters, int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes,
               int64_t chunk, hipStream_t st) {
    RALD_CHECK(grid.lo && grid.v && grid.dims, who + ": null grid (lo3, v3, dims3)");
    RALD_CHECK(std::isfinite(eps) && eps > 0.f, who + ": eps must be finite and > 0");
    for (int k = 0; k < 3; ++k) RALD_CHECK(grid.v[k] >= eps, who + ": every cell edge must be >= eps");   // NaN fails
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, cluster_scratch_bytes(c.batch, c.n_total, c.max_per_sample, chunk)));
    RALD_TRY(cloud_grid_check(who, c, grid, chunk, &a.g));
    a.c = c;
    CloudIndex ix;
    Carver s{(char*)scratch, 0};
    clu_layout(a, ix, s, chunk);
    if (out_labels) a.labels = out_labels;
    if (out_num_clusters) a.nclu = out_num_clusters;
    if (out_sizes) a.sizes = out_sizes;
    if (out_count) a.cnt = out_count;
    a.r2 = eps * eps;
    a.rs = scan_reach(eps);
    a.min_points = min_points;
    const SortedCloud sorted = cloud_index_build(ix, a.g, nullptr, st);
    a.skey = sorted.key; a.srow = sorted.rows;
    const dim3 by_row((unsigned)((c.max_per_sample + CLU_T - 1) / CLU_T), c.batch);
    const dim3 by_seg((unsigned)a.num.nseg_max, c.batch);
    hipLaunchKernelGGL(clu_init, by_row, dim3(CLU_T), 0, st, a);
    if (min_points > 0) hipLaunchKernelGGL(clu_count, by_row, dim3(CLU_T), 0, st, a);
    hipLaunchKernelGGL(clu_link, by_row, dim3(CLU_T), 0, st, a);
    hipLaunchKernelGGL(clu_flatten, by_seg, dim3(CLOUD_SEG), 0, st, a);
    block_scan_launch(c, a.num, st);
    hipLaunchKernelGGL(clu_number, by_seg, dim3(CLOUD_SEG), 0, st, a);
    hipLaunchKernelGGL(clu_label, by_row, dim3(CLU_T), 0, st, a);
    return 0;
}

}  // namespace

int64_t cluster_scratch_bytes(int B, int64_t n_total, int64_t max_per_sample, int64_t chunk) {
    return layout_bytes<ClusterArgs>(B, n_total, max_per_sample, chunk, clu_layout);
}

int cluster_labels_ragged(const RaggedCloud& c, const GridSpec& grid, float eps, int min_points, int32_t* out_labels, int32_t* out_num_clusters,
                          int32_t* out_sizes, int32_t* out_count, void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_labels && out_num_clusters, "cluster_labels_ragged: null pointer (points, out_labels, out_num_clusters)");
    RALD_CHECK(min_points >= 0, "cluster_labels_ragged: min_points must be >= 0");
    ClusterArgs a{};
    RALD_TRY(clu_labels("cluster_labels_ragged", a, c, grid, eps, min_points, out_labels, out_num_clusters, out_sizes, out_count, scratch,
                        scratch_bytes, chunk, st));
    RALD_HIP(hipGetLastError());
    return 0;
}

int cluster_filter_ragged(const RaggedCloud& c, const GridSpec& grid, float eps, int min_points, int min_cluster_size, int largest_only,
                          float* out_points, int64_t* out_offsets, int64_t* out_index, int32_t* out_labels, int32_t* out_num_clusters,
                          void* scratch, int64_t scratch_bytes, int64_t chunk, hipStream_t st) {
    RALD_CHECK(c.points && out_points && out_offsets && out_labels && out_num_clusters,
               "cluster_filter_ragged: null pointer (points, out_points, out_offsets, out_labels, out_num_clusters)");
    RALD_CHECK(min_points >= 0, "cluster_filter_ragged: min_points must be >= 0");
    RALD_CHECK(min_cluster_size >= 1, "cluster_filter_ragged: min_cluster_size must be >= 1");
    ClusterArgs a{};
    RALD_TRY(clu_labels("cluster_filter_ragged", a, c, grid, eps, min_points, nullptr, out_num_clusters, nullptr, nullptr, scratch, scratch_bytes,
                        chunk, st));
    a.min_size = min_cluster_size;
    a.largest = largest_only != 0;
    if (out_index) a.kept = out_index;
    a.sc.out_offsets = out_offsets;
    const dim3 by_row((unsigned)((c.max_per_sample + CLU_T - 1) / CLU_T), c.batch);
    if (a.largest) hipLaunchKernelGGL(clu_argmax, dim3(c.batch), dim3(CLU_T), 0, st, a);
    hipLaunchKernelGGL(clu_keep, by_row, dim3(CLU_T), 0, st, a);
    compact_rows_ragged(c, a.sc, a.root, 1, out_points, a.kept, st);
    cloud_kept_labels_ragged(c, out_offsets, a.kept, a.labels, out_labels, st);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
