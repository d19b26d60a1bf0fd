// meshsdf.hip -- mesh-to-level-set rasterisation (include/open/manta_hip_meshsdf.h): sources as count -> scan -> emit with one wave per
// triangle (lanes over the rows of the barycentric loop), a stable binning by cell (atomic counts, scan, radix sort of (cell, source)
// pairs), the gather with one thread per cell and lanes along x, and the flood fill as tile-local fixed points in LDS repeated until a
// launch changes nothing.  The per-item bodies are in meshsdf_cells.h.  Reference: mesh.cpp:769-1005, plugin/initplugins.cpp:132-152.
#include "meshsdf_cells.h"
#include "../../include/open/manta_hip_meshsdf.h"
#include "scan.h"

using namespace mf;
using namespace mf::meshsdf;

namespace {

constexpr int TRIS_PER_BLOCK = BLOCK / 64;
constexpr int FLOOD_THREADS = TILE * TILE * TILE;

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int u = __shfl_up(v, o, 64);
		if (lane >= o) v += u;
	}
	return v;
}

// res[0] |= 1: a node index outside the array, res[0] |= 2: a sample count that a short does not hold
__global__ void __launch_bounds__(BLOCK) k_src_count(TriView T, int64_t* __restrict__ cnt, int32_t* __restrict__ res) {
	const int64_t t = blockIdx.x * (int64_t)TRIS_PER_BLOCK + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (t >= T.nTris) return;
	V3 p[3];
	if (!tri_nodes(T, t, p)) {
		if (lane == 0) {
			cnt[t] = 0;
			atomicOr(res, 1);
		}
		return;
	}
	const Plan P = tri_plan(p);
	int c = 0;
	for (int s0 = lane; s0 < P.iterA; s0 += 64) c += row_count(P, s0);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
	if (lane == 0) {
		cnt[t] = 1 + (int64_t)c;
		if (P.wrap) atomicOr(res, 2);
	}
}

__global__ void k_src_total(int64_t n, const int64_t* __restrict__ off, const int64_t* __restrict__ last, int64_t* __restrict__ res) {
	if (blockIdx.x || threadIdx.x) return;
	res[1] = off[n - 1] + last[0];
}
// the scan is in place, so the last triangle's count is put aside first
__global__ void k_src_keep_last(int64_t n, const int64_t* __restrict__ cnt, int64_t* __restrict__ last) {
	if (blockIdx.x || threadIdx.x) return;
	last[0] = cnt[n - 1];
}

__global__ void __launch_bounds__(BLOCK) k_src_emit(TriView T, const int64_t* __restrict__ off, SrcOut S) {
	const int64_t t = blockIdx.x * (int64_t)TRIS_PER_BLOCK + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (t >= T.nTris) return;
	V3 p[3];
	if (!tri_nodes(T, t, p)) return;
	const Plan P = tri_plan(p);
	const V3 n = face_normal(p);
	int64_t run = off[t];
	if (lane == 0) put_source(S, run, face_centre(p, S), n);
	run++;
	for (int base = 0; base < P.iterA; base += 64) {
		const int s0 = base + lane;
		const int c = s0 < P.iterA ? row_count(P, s0) : 0;
		const int incl = wave_incl_scan(c, lane);
		if (s0 < P.iterA) emit_row(P, p, n, s0, run + (incl - c), S);
		run += __shfl(incl, 63, 64);
	}
}

__global__ void __launch_bounds__(BLOCK)
k_bin_key(Dim d, int64_t nSrc, int64_t scap, const float* __restrict__ spos, uint32_t* __restrict__ key, int32_t* __restrict__ val,
          int32_t* __restrict__ len, int32_t* __restrict__ occ) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= nSrc) return;
	const float x = spos[s], y = spos[scap + s], z = spos[2 * scap + s];
	const int64_t c = cell_index(d, x, y, z);
	key[s] = c < 0 ? (uint32_t)d.n : (uint32_t)c;
	val[s] = (int32_t)s;
	if (c >= 0) {
		atomicAdd(&len[c], 1);
		occ[occ_index(d, (int)x, (int)y, (int)z)] = 1;
	}
}

__global__ void __launch_bounds__(BLOCK)
k_bin_reorder(int64_t n, int64_t nSrc, int64_t scap, const uint32_t* __restrict__ key, const int32_t* __restrict__ val,
              const float* __restrict__ spos, const float* __restrict__ snrm, float* __restrict__ bpos, float* __restrict__ bnrm) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= nSrc || key[s] >= (uint32_t)n) return;
	const int64_t v = val[s];
	if (v < 0 || v >= nSrc) return;
	for (int c = 0; c < 3; c++) {
		bpos[c * scap + s] = spos[c * scap + v];
		bnrm[c * scap + s] = snrm[c * scap + v];
	}
}

__global__ void k_bin_total(int64_t n, const int32_t* __restrict__ len, const int32_t* __restrict__ start, int32_t* __restrict__ stats) {
	if (blockIdx.x || threadIdx.x) return;
	stats[0] = start[n - 1] + len[n - 1];
}

__global__ void __launch_bounds__(BLOCK) k_meshsdf_gather(Dim d, Gather G, float* __restrict__ phi) {
	CELL_IJK(d)
	phi[idx] = gather_cell(d, G, i, j, k);
}

__global__ void __launch_bounds__(BLOCK) k_flood_seed(int64_t n, float* __restrict__ phi, float cutoff) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (phi[idx] >= cutoff - 1.0f) phi[idx] = cutoff;
}

// One tile: propagate to the fixed point with the halo as it was read; the cells that flooded are written and the tile reports in.  A
// halo value that another tile changes during this launch may or may not be seen: a cell only ever goes from candidate to flooded, so a
// missed change is caught by the next launch, and the launch that changes nothing has read a settled field.
__global__ void __launch_bounds__(FLOOD_THREADS) k_flood_round(Dim d, float* __restrict__ phi, float cutoff, int32_t* __restrict__ changedTiles) {
	__shared__ int st[HALO * HALO * HALO];
	const int tid = threadIdx.x;
	const int ox = blockIdx.x * TILE, oy = blockIdx.y * TILE, oz = blockIdx.z * TILE;
	for (int s = tid; s < HALO * HALO * HALO; s += FLOOD_THREADS) st[s] = flood_state(d, phi, cutoff, ox, oy, oz, s);
	__syncthreads();
	const int lx = tid % TILE, ly = (tid / TILE) % TILE, lz = tid / (TILE * TILE);
	const int slot = (lx + 1) + HALO * (ly + 1) + HALO * HALO * (lz + 1);
	if (!__syncthreads_or(st[slot] == 1)) return;      // no candidate in the tile (uniform)
	bool changed = false;
	for (;;) {
		const bool ch = flood_step(st, slot);
		__syncthreads();                                 // every read of this sweep precedes its writes
		if (ch) {
			st[slot] = 2;
			changed = true;
		}
		if (!__syncthreads_or(ch)) break;
	}
	if (changed) phi[(int64_t)(ox + lx) + d.Y * (oy + ly) + d.Z * (oz + lz)] = cutoff;     // a candidate lies inside the grid
	if (__syncthreads_or(changed) && tid == 0) atomicAdd(changedTiles, 1);
}

template <class T>
__global__ void __launch_bounds__(BLOCK)
k_apply(Dim d, const float* __restrict__ sdf, const int32_t* __restrict__ flags, int ncomp, T* __restrict__ grid, T v0, T v1, T v2) {
	CELL_IJK(d)
	if (flags && (flags[idx] & 2)) return;       // FlagGrid::TypeObstacle
	if (sdf[idx] < 0.f) {
		grid[idx] = v0;
		if (ncomp == 3) {
			grid[d.n + idx] = v1;
			grid[2 * d.n + idx] = v2;
		}
	}
}

__global__ void __launch_bounds__(BLOCK)
k_apply_density(Dim d, const int32_t* __restrict__ flags, float* __restrict__ density, const float* __restrict__ sdf, float value, float sigma) {
	CELL_IJK(d)
	if (!(flags[idx] & 1) || sdf[idx] > sigma) return;      // FlagGrid::TypeFluid
	density[idx] = value;
}

int check_grid(const char* who, int sx, int sy, int sz) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sz == 1) return fail("%s: 3-D grids only", who);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}
int check_mesh(const char* who, int64_t nTris, int64_t tcap, int64_t nNodes, int64_t ncap) {
	if (nTris < 0 || tcap < nTris || nNodes < 0 || ncap < nNodes)
		return fail("%s: %lld triangles / %lld nodes in arrays of stride %lld / %lld", who, (long long)nTris, (long long)nNodes, (long long)tcap, (long long)ncap);
	if (nTris >= (int64_t)1 << 31) return fail("%s: too many triangles", who);
	return 0;
}
// the largest workspace of the source-offset scan (nTris), the cell-start scan (nCells) and the source sort (nSrc), behind the head.
// The errors of the queries (no device) are passed over: mf_meshsdf_tmp_bytes answers without a GPU, and the entries that use the
// scratch fail at their first launch there
int64_t tmp_need(int64_t nTris, int64_t nSrc, int64_t nCells) {
	size_t b = 0;
	if (nTris > 0) (void)exclusive_sum64_bytes(nTris, &b);
	if (nCells > 0) (void)exclusive_sum32_bytes(nCells, &b);
	if (nSrc > 0) (void)sort_pairs_bytes(nSrc, key_bits(nCells), &b);
	return head_ws_bytes(b);
}

}  // namespace

extern "C" {

int mf_meshsdf_abi_version(void) { return MF_MESHSDF_ABI_VERSION; }

int mf_meshsdf_tmp_bytes(int64_t nTris, int64_t nSrc, int64_t nCells, int64_t* bytes_host) {
	if (nTris < 0 || nSrc < 0 || nCells < 0 || nTris >= (int64_t)1 << 31 || nSrc >= (int64_t)1 << 31 || nCells >= (int64_t)1 << 31)
		return fail("meshSDF: %lld triangles, %lld sources, %lld cells", (long long)nTris, (long long)nSrc, (long long)nCells);
	*bytes_host = tmp_need(nTris, nSrc, nCells);
	return 0;
}

int mf_meshsdf_plan(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, int64_t* off, void* tmp,
                    int64_t tmp_bytes, int64_t* total_host, void* stream) {
	MF_TRY(check_mesh("meshSDF", nTris, tcap, nNodes, ncap));
	*total_host = 0;
	if (nTris == 0) return 0;
	const int64_t need = tmp_need(nTris, 0, 0);
	const hipStream_t st = (hipStream_t)stream;
	// the head of tmp: res[0] the flags of k_src_count (its low int), res[1] the total, res[2] the last triangle's count
	HeadWs t;
	MF_TRY(head_ws_cut("meshSDF", tmp, tmp_bytes, need, &t));
	int64_t* res = t.head;
	const TriView T = {nTris, tcap, nNodes, ncap, tri, pos};
	MF_HIP(hipMemsetAsync(res, 0, 256, st));
	hipLaunchKernelGGL(k_src_count, dim3((unsigned)((nTris + TRIS_PER_BLOCK - 1) / TRIS_PER_BLOCK)), dim3(BLOCK), 0, st, T, off, (int32_t*)res);
	hipLaunchKernelGGL(k_src_keep_last, dim3(1), dim3(64), 0, st, nTris, (const int64_t*)off, res + 2);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, off, off, nTris, st));
	hipLaunchKernelGGL(k_src_total, dim3(1), dim3(64), 0, st, nTris, (const int64_t*)off, (const int64_t*)(res + 2), res);
	MF_LAUNCH_CHECK();
	int64_t host[2] = {0, 0};
	MF_TRY(read_back(host, res, sizeof(host), st));
	if (host[0] & 1) return fail("meshSDF: a triangle names a node outside the mesh's %lld nodes", (long long)nNodes);
	if (host[0] & 2) return fail("meshSDF: a triangle edge of 43690 units or more: its sample count does not fit the reference's short");
	if (host[1] >= (int64_t)1 << 31) return fail("meshSDF: %lld sources do not fit 32-bit source numbers", (long long)host[1]);
	*total_host = host[1];
	return 0;
}

int mf_meshsdf_emit(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const int64_t* off,
                    int64_t total, float mx, float my, float mz, int64_t scap, float* spos, float* snrm, void* stream) {
	MF_TRY(check_mesh("meshSDF", nTris, tcap, nNodes, ncap));
	if (total < nTris || scap < total) return fail("meshSDF: %lld sources of %lld triangles in arrays of stride %lld", (long long)total, (long long)nTris, (long long)scap);
	if (nTris == 0) return 0;
	const TriView T = {nTris, tcap, nNodes, ncap, tri, pos};
	const SrcOut S = {total, scap, spos, snrm, mx, my, mz};
	hipLaunchKernelGGL(k_src_emit, dim3((unsigned)((nTris + TRIS_PER_BLOCK - 1) / TRIS_PER_BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, T, off, S);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshsdf_bin(int sx, int sy, int sz, int64_t nSrc, int64_t scap, const float* spos, const float* snrm, int32_t* keys, float* bpos,
                   float* bnrm, int32_t* len, int32_t* start, int32_t* occ, int32_t* stats, void* tmp, int64_t tmp_bytes, void* stream) {
	MF_TRY(check_grid("meshSDF", sx, sy, sz));
	if (nSrc < 0 || scap < nSrc || nSrc >= (int64_t)1 << 31) return fail("meshSDF: %lld sources in arrays of stride %lld", (long long)nSrc, (long long)scap);
	const Dim d = mkdim(sx, sy, sz);
	const int64_t need = tmp_need(0, nSrc, d.n);
	const hipStream_t st = (hipStream_t)stream;
	HeadWs t;   // the binning leaves the head alone
	MF_TRY(head_ws_cut("meshSDF", tmp, tmp_bytes, need, &t));
	const int64_t nocc = (int64_t)occ_dim(sx) * occ_dim(sy) * occ_dim(sz);
	MF_HIP(hipMemsetAsync(len, 0, d.n * sizeof(int32_t), st));
	MF_HIP(hipMemsetAsync(occ, 0, nocc * sizeof(int32_t), st));
	uint32_t* key = (uint32_t*)keys;
	int32_t* val = keys + scap;
	uint32_t* key2 = (uint32_t*)(keys + 2 * scap);
	int32_t* val2 = keys + 3 * scap;
	if (nSrc > 0) {
		hipLaunchKernelGGL(k_bin_key, dim3(nblk(nSrc)), dim3(BLOCK), 0, st, d, nSrc, scap, spos, key, val, len, occ);
		MF_LAUNCH_CHECK();
	}
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, len, start, d.n, st));
	hipLaunchKernelGGL(k_bin_total, dim3(1), dim3(64), 0, st, d.n, (const int32_t*)len, (const int32_t*)start, stats);
	MF_LAUNCH_CHECK();
	if (nSrc > 0) {
		// stable: within a cell the sources keep their order; the dropped ones (key n) come last
		MF_TRY(sort_pairs(t.ws, t.ws_bytes, key, key2, val, val2, nSrc, key_bits(d.n), st));
		hipLaunchKernelGGL(k_bin_reorder, dim3(nblk(nSrc)), dim3(BLOCK), 0, st, d.n, nSrc, scap, (const uint32_t*)key2, (const int32_t*)val2, spos,
		                   snrm, bpos, bnrm);
		MF_LAUNCH_CHECK();
	}
	return 0;
}

int mf_meshsdf_gather(int sx, int sy, int sz, int64_t scap, const float* bpos, const float* bnrm, const int32_t* len, const int32_t* start,
                      const int32_t* occ, float sigma, float cutoff, float* phi, void* stream) {
	MF_TRY(check_grid("meshSDF", sx, sy, sz));
	if (!(sigma > 0.f)) return fail("meshSDF: sigma must be positive");
	const Dim d = mkdim(sx, sy, sz);
	const Gather G = {bpos, bnrm, scap, len, start, occ, make_params(sigma, cutoff)};
	hipLaunchKernelGGL(k_meshsdf_gather, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, G, phi);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshsdf_flood(int sx, int sy, int sz, float* phi, float sigma, float cutoff, int flood, int32_t* stats, int32_t* out_host, void* stream) {
	MF_TRY(check_grid("meshSDF", sx, sy, sz));
	if (!(sigma > 0.f)) return fail("meshSDF: sigma must be positive");
	const Dim d = mkdim(sx, sy, sz);
	const float c = make_params(sigma, cutoff).cutoff;
	const hipStream_t st = (hipStream_t)stream;
	out_host[0] = 0;
	int32_t host[2] = {0, 0};
	if (!flood) {
		MF_TRY(read_back(host, stats, sizeof(host), st));
		out_host[1] = host[0];
		return 0;
	}
	hipLaunchKernelGGL(k_flood_seed, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d.n, phi, c);
	MF_LAUNCH_CHECK();
	const dim3 tiles((sx + TILE - 1) / TILE, (sy + TILE - 1) / TILE, (sz + TILE - 1) / TILE);
	// a round that changes something floods at least one cell, so n + 1 rounds always suffice
	for (int64_t round = 0; round <= d.n; round++) {
		MF_HIP(hipMemsetAsync(stats + 1, 0, sizeof(int32_t), st));
		hipLaunchKernelGGL(k_flood_round, tiles, dim3(FLOOD_THREADS), 0, st, d, phi, c, stats + 1);
		MF_LAUNCH_CHECK();
		MF_TRY(read_back(host, stats, sizeof(host), st));
		out_host[0]++;
		if (host[1] == 0) break;
	}
	out_host[1] = host[0];
	return 0;
}

int mf_meshsdf_apply(int sx, int sy, int sz, const float* sdf, const int32_t* flags, int kind, void* grid, int ivalue, float vx, float vy,
                     float vz, void* stream) {
	MF_TRY(check_grid("Mesh::applyMeshToGrid", sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	if (kind == 0)
		hipLaunchKernelGGL(k_apply<int32_t>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, sdf, flags, 1, (int32_t*)grid, ivalue, 0, 0);
	else if (kind == 1 || kind == 2)
		hipLaunchKernelGGL(k_apply<float>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, sdf, flags, kind == 2 ? 3 : 1, (float*)grid, vx, vy, vz);
	else
		return fail("Shape::applyToGrid(): unknown grid type");
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshsdf_apply_density(int sx, int sy, int sz, const int32_t* flags, float* density, const float* sdf, float value, float sigma,
                             void* stream) {
	MF_TRY(check_grid("densityInflowMesh", sx, sy, sz));
	hipLaunchKernelGGL(k_apply_density, dim3(nblk(mkdim(sx, sy, sz).n)), dim3(BLOCK), 0, (hipStream_t)stream, mkdim(sx, sy, sz), flags, density, sdf,
	                   value, sigma);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
