// Isosurface meshing of a batch of dense float volumes by naive surface nets: one vertex per sign-changing cell,
// one quad (two triangles) per sign-changing grid edge that has four cells around it.  The definition is in include/rald_hip.h; in short
//   INSIDE   value > iso (a NaN is outside)
//   vertex   of an active cell: the mean, in cell units, of the crossing points of its 12 edges in ascending e = 4 axis + 2 p + q,
//            t = fl(fl(iso - a) / fl(b - a)), NaN -> 0, clamped into [0, 1]; fl(lo + fl(fl((float)i + u) * h)) per axis; fp32, no contraction
//   order    vertices by ascending cell index, faces by ascending ((i ny + j) nz + k) 3 + axis of the edge's lower node
// Everything before the emit runs on sign bits: a WORD is the 64 INSIDE bits of one z-run of 64 nodes, word (i, j, w) of a volume at
// (i ny + j) W + w with W = ceil(nz / 64), bit z % 64.  Cell (i, j, k) and the three edges that leave node (i, j, k) belong to word
// (i, j, k / 64): the active cells of a word are `any & ~all` over the words of the four rows around it and their one-bit shifts, the
// crossing edges are XORs of the same words, the counts are popcounts, and the scans run over words.
// Launches, all on one stream, none waits on another workgroup, no atomics:
//   sn_bits      one wave per 4 words              the volume, read once and coalesced along z -> the words (1 / 32 of the volume)
//   sn_count     (1024 words, volume)              the active mask and the face-edge mask of every word, its vertex and triangle counts,
//                                                  their exclusive prefix inside the workgroup and the workgroup's totals
//   the two block scans of cloud_index.hip, once for the vertices and once for the triangles: the offsets over the batch, TRUE counts
//   sn_vertices  one wave per word, lane = cell    the vertex of every active cell (eight loads a cell), its cell index; a wave whose
//                                                  word holds nothing leaves after one load
//   sn_faces     one wave per word, lane = node    the two triangles of every crossing edge; a cell's vertex id is its word's base plus
//                                                  the popcount of the word's active mask below its bit
// Every loop is bounded by 4, 12, SN_EW or the number of waves.  Every index that comes from the scratch (a word's base, a block's base, the
// offsets) is checked against the capacity before it addresses a row; the masks read back from the scratch are cut to the cells and
// nodes of the grid before a lane reads the volume by them.
#include "cloud_index.h"
#include "kernels.h"

namespace rald {

namespace {

constexpr int SN_T = 256;                                    // threads of the per-wave kernels: four waves
constexpr int SN_WPW = 4;                                    // words per wave of sn_bits
constexpr int SN_EW = 1;                                     // words per wave of the emit kernels; timed at 1, 4 and 16: a wave
                                                             // that walks several words in turn loses more than the empty words' waves cost
constexpr int64_t SN_MAX_NODES = (((int64_t)1 << 31) - 1) / 6;   // batch * nx * ny * nz: six triangles a node at most, counted in int32

struct SurfArgs {
    RaggedCloud c;                                           // the words as the rows of a dense batch: what the block scans walk
    const float* vol;
    int nx, ny, nz, W;
    int64_t nwords, nodes, total_words;                      // per volume, per volume, over the batch
    float iso, lo[3], h[3];
    unsigned long long* bits;                                // [batch][nwords] INSIDE
    unsigned long long* act;                                 // [batch][nwords] the active cells
    unsigned long long* edges;                               // [batch][nwords] the nodes with an edge that makes a face: what sn_faces skips by
    int* vpre; int* fpre;                                    // [batch][nwords] vertices / triangles before the word inside its block of 1024
    BlockScan vs, fs;
    float* out_vertices; int32_t* out_faces; int32_t* out_cells;
    int64_t max_vertices, max_faces;
};

__device__ __forceinline__ unsigned long long sn_word(const SurfArgs& a, const unsigned long long* vb, int i, int j, int w) {
    return w < a.W ? vb[((int64_t)i * a.ny + j) * a.W + w] : 0ull;
}
// the word and, shifted down by one bit, the bits of the nodes one above in z
__device__ __forceinline__ void sn_pair(const SurfArgs& a, const unsigned long long* vb, int i, int j, int w, unsigned long long& r,
                                        unsigned long long& s) {
    r = sn_word(a, vb, i, j, w);
    s = (r >> 1) | (sn_word(a, vb, i, j, w + 1) << 63);
}
// bits k of word w with w * 64 + k < nz - 1: the cells of a row, and the nodes that have a node above them
__device__ __forceinline__ unsigned long long sn_cells(const SurfArgs& a, int w) {
    const int nc = a.nz - 1 - w * 64;
    return nc >= 64 ? ~0ull : (nc <= 0 ? 0ull : (1ull << nc) - 1ull);
}
// the masks of word (i, j, w) of the volume whose words are vb: the active cells, and per axis the nodes whose edge makes a face
__device__ __forceinline__ void sn_masks(const SurfArgs& a, const unsigned long long* vb, int i, int j, int w, unsigned long long& act,
                                         unsigned long long* X) {
    unsigned long long r00, s00;
    sn_pair(a, vb, i, j, w, r00, s00);
    const unsigned long long cm = sn_cells(a, w);
    const unsigned long long km = w == 0 ? cm & ~1ull : cm;   // 1 <= k <= nz - 2
    const bool xi = i >= 1 && i <= a.nx - 2, yi = j >= 1 && j <= a.ny - 2, xn = i + 1 < a.nx, yn = j + 1 < a.ny;
    const unsigned long long r10 = xn ? sn_word(a, vb, i + 1, j, w) : 0ull, r01 = yn ? sn_word(a, vb, i, j + 1, w) : 0ull;
    X[0] = xn && yi ? (r00 ^ r10) & km : 0ull;
    X[1] = yn && xi ? (r00 ^ r01) & km : 0ull;
    X[2] = xi && yi ? (r00 ^ s00) & cm : 0ull;
    act = 0ull;
    if (xn && yn) {
        unsigned long long r11, s11;
        const unsigned long long s10 = (r10 >> 1) | (sn_word(a, vb, i + 1, j, w + 1) << 63);
        const unsigned long long s01 = (r01 >> 1) | (sn_word(a, vb, i, j + 1, w + 1) << 63);
        sn_pair(a, vb, i + 1, j + 1, w, r11, s11);
        const unsigned long long any = r00 | s00 | r10 | s10 | r01 | s01 | r11 | s11;
        const unsigned long long all = r00 & s00 & r10 & s10 & r01 & s01 & r11 & s11;
        act = any & ~all & cm;
    }
}
// word g of a volume -> (i, j, w); g < 2^24: 32-bit divisions
__device__ __forceinline__ void sn_split(const SurfArgs& a, int64_t g, int& i, int& j, int& w) {
    const unsigned g32 = (unsigned)g, row = g32 / (unsigned)a.W;
    w = (int)(g32 - row * (unsigned)a.W);
    i = (int)(row / (unsigned)a.ny);
    j = (int)(row - (unsigned)i * (unsigned)a.ny);
}
// the words of an emit wave that hold something, as a mask over the wave's SN_EW words from gw0 on; flags: act or edges
__device__ __forceinline__ unsigned long long sn_todo(const SurfArgs& a, const unsigned long long* flags, int64_t gw0, int lane) {
    const bool mine = lane < SN_EW && gw0 + lane < a.total_words && flags[gw0 + lane] != 0ull;
    return __ballot(mine);
}

__global__ __launch_bounds__(SN_T) void sn_bits(SurfArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (SN_T / 64) + (threadIdx.x >> 6);
    float v[SN_WPW];
    bool on[SN_WPW];
#pragma unroll
    for (int r = 0; r < SN_WPW; ++r) {                       // the loads first: four z-runs in flight a wave
        const int64_t gw = wave * SN_WPW + r;
        on[r] = gw < a.total_words;
        v[r] = NAN;
        if (on[r]) {
            const int64_t b = gw / a.nwords, g = gw - b * a.nwords, row = g / a.W;
            const int z = (int)(g - row * a.W) * 64 + lane;
            if (z < a.nz) v[r] = a.vol[b * a.nodes + row * a.nz + z];
        }
    }
#pragma unroll
    for (int r = 0; r < SN_WPW; ++r) {
        const unsigned long long m = __ballot(v[r] > a.iso);  // a NaN, and a lane behind nz, is outside
        if (on[r] && lane == 0) a.bits[wave * SN_WPW + r] = m;
    }
}

__global__ __launch_bounds__(CLOUD_SEG) void sn_count(SurfArgs a) {
    __shared__ int sh[CLOUD_SEG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * CLOUD_SEG + tid;
    int nv = 0, nf = 0;
    if (g < a.nwords) {
        int i, j, w;
        sn_split(a, g, i, j, w);
        unsigned long long act, X[3];
        sn_masks(a, a.bits + (int64_t)b * a.nwords, i, j, w, act, X);
        a.act[(int64_t)b * a.nwords + g] = act;
        a.edges[(int64_t)b * a.nwords + g] = X[0] | X[1] | X[2];
        nv = __popcll(act);
        nf = 2 * (__popcll(X[0]) + __popcll(X[1]) + __popcll(X[2]));
    }
    int tv, tf;                                              // every thread of the workgroup reaches both scans
    const int ev = vox_block_excl<CLOUD_SEG>(nv, sh, tid, &tv);
    const int ef = vox_block_excl<CLOUD_SEG>(nf, sh, tid, &tf);
    if (g < a.nwords) {
        a.vpre[(int64_t)b * a.nwords + g] = ev;
        a.fpre[(int64_t)b * a.nwords + g] = ef;
    }
    if (tid == 0) {
        a.vs.blocks[(int64_t)b * a.vs.nseg_max + blockIdx.x] = tv;
        a.fs.blocks[(int64_t)b * a.fs.nseg_max + blockIdx.x] = tf;
    }
}

// the vertex of cell (i, j, k) of the volume v (its node (0, 0, 0)), in fp32 without contraction
__device__ __forceinline__ void sn_vertex(const SurfArgs& a, const float* v, int i, int j, int k, float* out) {
#pragma clang fp contract(off)
    float c[2][2][2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) c[dx][dy][dz] = v[(((int64_t)(i + dx)) * a.ny + (j + dy)) * a.nz + (k + dz)];
    float s[3] = {0.f, 0.f, 0.f};
    int count = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int axis = e >> 2, p = (e >> 1) & 1, q = e & 1;
        const int o1 = axis == 0 ? 1 : 0, o2 = axis == 2 ? 1 : 2;   // the two other axes, ascending
        int d0[3], d1[3];
        d0[axis] = 0; d1[axis] = 1;
        d0[o1] = d1[o1] = p;
        d0[o2] = d1[o2] = q;
        const float va = c[d0[0]][d0[1]][d0[2]], vb = c[d1[0]][d1[1]][d1[2]];
        if ((va > a.iso) != (vb > a.iso)) {
            float t = (a.iso - va) / (vb - va);
            t = t != t ? 0.f : t;
            t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
            s[axis] += t;
            s[o1] += (float)p;
            s[o2] += (float)q;
            ++count;
        }
    }
    const float n = (float)count;                            // >= 1: the cell is active
    const int at[3] = {i, j, k};
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const float u = s[x] / n;
        out[x] = a.lo[x] + ((float)at[x] + u) * a.h[x];
    }
}

// the first row of volume b in an output of `cap` rows, or -1 when the offset is outside 0 .. 2^62 (the scratch was not what the scans left)
__device__ __forceinline__ int64_t sn_row0(const int64_t* offsets, int b) {
    const int64_t o = offsets[b];
    return o < 0 || o > ((int64_t)1 << 62) ? -1 : o;
}

__global__ __launch_bounds__(SN_T) void sn_vertices(SurfArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t gw0 = ((int64_t)blockIdx.x * (SN_T / 64) + (threadIdx.x >> 6)) * SN_EW;
    if (gw0 >= a.total_words) return;                        // the whole wave
    unsigned long long todo = sn_todo(a, a.act, gw0, lane);
    for (int it = 0; it < SN_EW && todo != 0ull; ++it) {     // the wave's words with an active cell, in turn; uniform
        const int64_t gw = gw0 + (__ffsll((long long)todo) - 1);
        todo &= todo - 1ull;
        const int64_t b = (int64_t)((unsigned)gw / (unsigned)a.nwords), g = gw - b * a.nwords;   // gw < 2^31
        int i, j, w;
        sn_split(a, g, i, j, w);
        if (i + 1 >= a.nx || j + 1 >= a.ny) continue;
        const unsigned long long m = a.act[gw] & sn_cells(a, w);   // cut to the row's cells: lane k reads nodes k and k + 1
        if (!((m >> lane) & 1ull)) continue;
        const int k = w * 64 + lane;
        const int64_t base = sn_row0(a.vs.out_offsets, (int)b);
        const int64_t vid = (int64_t)a.vs.blocks[b * a.vs.nseg_max + g / CLOUD_SEG] + a.vpre[gw] + __popcll(m & vox_lanes_below(lane));
        const int64_t row = base + vid;
        if (base < 0 || vid < 0 || row >= a.max_vertices) continue;
        if (a.out_vertices) {
            float p[3];
            sn_vertex(a, a.vol + b * a.nodes, i, j, k, p);
            a.out_vertices[row * 3] = p[0]; a.out_vertices[row * 3 + 1] = p[1]; a.out_vertices[row * 3 + 2] = p[2];
        }
        if (a.out_cells) a.out_cells[row] = (int32_t)(((int64_t)i * (a.ny - 1) + j) * (a.nz - 1) + k);
    }
}

// the vertex of cell (i, j, k) of volume b, numbered inside the volume; the cell exists
__device__ __forceinline__ int32_t sn_vid(const SurfArgs& a, int64_t b, int i, int j, int k) {
    const int64_t g = ((int64_t)i * a.ny + j) * a.W + (k >> 6);
    const int64_t gw = b * a.nwords + g;
    return a.vs.blocks[b * a.vs.nseg_max + g / CLOUD_SEG] + a.vpre[gw] + __popcll(a.act[gw] & vox_lanes_below(k & 63));
}

__global__ __launch_bounds__(SN_T) void sn_faces(SurfArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t gw0 = ((int64_t)blockIdx.x * (SN_T / 64) + (threadIdx.x >> 6)) * SN_EW;
    if (gw0 >= a.total_words) return;                        // the whole wave
    unsigned long long todo = sn_todo(a, a.edges, gw0, lane);
    for (int it = 0; it < SN_EW && todo != 0ull; ++it) {     // the wave's words with a face, in turn; uniform
        const int64_t gw = gw0 + (__ffsll((long long)todo) - 1);
        todo &= todo - 1ull;
        const int64_t b = (int64_t)((unsigned)gw / (unsigned)a.nwords), g = gw - b * a.nwords;   // gw < 2^31
        int i, j, w;
        sn_split(a, g, i, j, w);
        const unsigned long long* vb = a.bits + b * a.nwords;
        unsigned long long act, X[3];
        sn_masks(a, vb, i, j, w, act, X);                    // from the sign words again: cut to the nodes whose four cells exist
        if (!(((X[0] | X[1] | X[2]) >> lane) & 1ull)) continue;
        const int k = w * 64 + lane;
        const bool inside = (sn_word(a, vb, i, j, w) >> lane) & 1ull;
        const unsigned long long below = vox_lanes_below(lane);
        const int64_t base = sn_row0(a.fs.out_offsets, (int)b);
        int64_t tri = (int64_t)a.fs.blocks[b * a.fs.nseg_max + g / CLOUD_SEG] + a.fpre[gw] +
                      2 * (__popcll(X[0] & below) + __popcll(X[1] & below) + __popcll(X[2] & below));
        if (base < 0 || tri < 0) continue;
        const int n[3] = {i, j, k};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((X[ax] >> lane) & 1ull)) continue;
            const int u = (ax + 1) % 3, v = (ax + 2) % 3;    // (y, z), (z, x), (x, y)
            const int64_t row = base + tri;
            tri += 2;
            if (row >= a.max_faces) continue;                // the second triangle lies behind the first
            int c[3] = {n[0], n[1], n[2]};
            c[u] -= 1; c[v] -= 1;
            const int32_t c0 = sn_vid(a, b, c[0], c[1], c[2]);
            c[u] += 1;
            const int32_t c1 = sn_vid(a, b, c[0], c[1], c[2]);
            c[v] += 1;
            const int32_t c2 = sn_vid(a, b, c[0], c[1], c[2]);
            c[u] -= 1;
            const int32_t c3 = sn_vid(a, b, c[0], c[1], c[2]);
            int32_t* f = a.out_faces + row * 3;
            f[0] = c0; f[1] = inside ? c1 : c2; f[2] = inside ? c2 : c1;
            if (row + 1 < a.max_faces) { f[3] = c0; f[4] = inside ? c2 : c3; f[5] = inside ? c3 : c2; }
        }
    }
}

bool sn_sizes_ok(int B, int nx, int ny, int nz) {
    if (B < 1 || B > 65535) return false;
    if (nx < 2 || nx > 1024 || ny < 2 || ny > 1024 || nz < 2 || nz > 1024) return false;
    return (int64_t)B * nx * ny * nz <= SN_MAX_NODES;
}

// the scratch, described once; the sizes of a are set
void sn_layout(SurfArgs& a, Carver& s) {
    const int64_t B = a.c.batch;
    a.bits = s.take<unsigned long long>(B * a.nwords);
    a.act = s.take<unsigned long long>(B * a.nwords);
    a.edges = s.take<unsigned long long>(B * a.nwords);
    a.vpre = s.take<int>(B * a.nwords);
    a.fpre = s.take<int>(B * a.nwords);
    block_scan_layout(a.vs, a.c, s);
    block_scan_layout(a.fs, a.c, s);
}

void sn_sizes(SurfArgs& a, int B, int nx, int ny, int nz) {
    a.nx = nx; a.ny = ny; a.nz = nz;
    a.W = (nz + 63) / 64;
    a.nwords = (int64_t)nx * ny * a.W;                       // <= 2^24: the block scans' bound on a cloud
    a.nodes = (int64_t)nx * ny * nz;
    a.total_words = a.nwords * B;
    a.c = ragged_cloud(nullptr, nullptr, nullptr, B, a.nwords, a.total_words, a.nwords);
}

const char* const SN_SIZES = "batch 1 .. 65535, dims 2 .. 1024 each, batch * nx * ny * nz <= 357913941";

}  // namespace

int64_t surface_scratch_bytes(int B, int nx, int ny, int nz) {
    if (!sn_sizes_ok(B, nx, ny, nz)) return -1;
    SurfArgs a{};
    sn_sizes(a, B, nx, ny, nz);
    Carver s{nullptr, 0};
    sn_layout(a, s);
    return s.used;
}

int surface_nets(const float* volume, int B, const int32_t* dims3_host, const float* lo3_host, const float* spacing3_host, float iso,
                 float* out_vertices, int64_t* out_v_offsets, int64_t max_vertices, int32_t* out_faces, int64_t* out_f_offsets,
                 int64_t max_faces, int32_t* out_cells, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    const std::string who = "surface_nets";
    RALD_CHECK(volume && dims3_host && lo3_host && spacing3_host && out_v_offsets && out_f_offsets,
               who + ": null pointer (volume, dims, lo, spacing, out_v_offsets, out_f_offsets)");
    RALD_CHECK(sn_sizes_ok(B, dims3_host[0], dims3_host[1], dims3_host[2]), who + ": " + SN_SIZES);
    for (int k = 0; k < 3; ++k) {
        RALD_CHECK(std::isfinite(spacing3_host[k]) && spacing3_host[k] > 0.f, who + ": spacing must be finite and > 0");
        RALD_CHECK(std::isfinite(lo3_host[k]), who + ": lo must be finite");
    }
    RALD_CHECK(!std::isnan(iso), who + ": iso must not be NaN");
    RALD_CHECK(max_vertices >= 0 && max_faces >= 0 && max_vertices <= ((int64_t)1 << 40) && max_faces <= ((int64_t)1 << 40),
               who + ": max_vertices and max_faces must be 0 .. 2^40");
    RALD_TRY(scratch_check(who, scratch, scratch_bytes, surface_scratch_bytes(B, dims3_host[0], dims3_host[1], dims3_host[2])));
    SurfArgs a{};
    sn_sizes(a, B, dims3_host[0], dims3_host[1], dims3_host[2]);
    Carver s{(char*)scratch, 0};
    sn_layout(a, s);
    a.vol = volume;
    a.iso = iso;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo3_host[k]; a.h[k] = spacing3_host[k]; }
    a.vs.out_offsets = out_v_offsets;
    a.fs.out_offsets = out_f_offsets;
    a.out_vertices = out_vertices; a.out_faces = out_faces; a.out_cells = out_cells;
    a.max_vertices = max_vertices; a.max_faces = max_faces;
    const unsigned by_wave = (unsigned)((a.total_words + SN_T / 64 * SN_EW - 1) / (SN_T / 64 * SN_EW));
    const unsigned by_run = (unsigned)((a.total_words + SN_T / 64 * SN_WPW - 1) / (SN_T / 64 * SN_WPW));
    hipLaunchKernelGGL(sn_bits, dim3(by_run), dim3(SN_T), 0, st, a);
    hipLaunchKernelGGL(sn_count, dim3((unsigned)a.vs.nseg_max, B), dim3(CLOUD_SEG), 0, st, a);
    block_scan_launch(a.c, a.vs, st);
    block_scan_launch(a.c, a.fs, st);
    if ((out_vertices || out_cells) && max_vertices > 0) hipLaunchKernelGGL(sn_vertices, dim3(by_wave), dim3(SN_T), 0, st, a);
    if (out_faces && max_faces > 0) hipLaunchKernelGGL(sn_faces, dim3(by_wave), dim3(SN_T), 0, st, a);
    RALD_HIP(hipGetLastError());
    return 0;
}

}  // namespace rald
