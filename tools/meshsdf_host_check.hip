// tools/meshsdf_host_check.hip -- the bodies of mantaflow_amd/csrc/meshsdf_cells.h run on the HOST: every launch of meshsdf.hip replaced
// by a serial loop (a wave's lanes by a loop over the rows, the scans and the sort by serial sums and a stable counting pass, a flood
// round by a loop over the tiles with each tile's sweep as decide-then-write), as a stand-alone program for the host sanitizers.
// tools/meshsdf_host_check.py drives it with every case of tests/meshsdf_model.py and compares each stage with the model.  It makes no
// HIP call and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/meshsdf_host_check.hip -o <scratch>/meshsdf_host_check
//   python tools/meshsdf_host_check.py <scratch>/meshsdf_host_check
//
// usage: meshsdf_host_check <in.bin> <out.bin>
//   in:  int32 sx, sy, sz, nNodes, nTris, flood-only; float mult[3], sigma, cutoff; pos[3][nNodes]; tri[3][nTris]; (flood-only: phi[n])
//   out: int64 nSrc, binned, rounds; spos[3][nSrc], snrm[3][nSrc]; len[n], start[n]; bpos[3][nSrc], bnrm[3][nSrc] (binned entries, rest 0);
//        pre[n]; phi[n]
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/meshsdf_cells.h"
#include <stdlib.h>

using namespace mf;
using namespace mf::meshsdf;

template <class T>
static T* exact(int64_t count) { return (T*)calloc(count ? count : 1, sizeof(T)); }

static int flood(const Dim& d, float* phi, float c) {
	for (int64_t i = 0; i < d.n; i++)
		if (phi[i] >= c - 1.0f) phi[i] = c;
	int rounds = 0;
	int* st = exact<int>(HALO * HALO * HALO);
	bool* ch = exact<bool>(TILE * TILE * TILE);
	float* next = exact<float>(d.n);
	for (;;) {
		rounds++;
		int changedTiles = 0;
		memcpy(next, phi, d.n * sizeof(float));          // every tile of a round reads the field as the round began
		for (int oz = 0; oz < d.sz; oz += TILE)
			for (int oy = 0; oy < d.sy; oy += TILE)
				for (int ox = 0; ox < d.sx; ox += TILE) {
					for (int s = 0; s < HALO * HALO * HALO; s++) st[s] = flood_state(d, phi, c, ox, oy, oz, s);
					bool changed = false;
					for (;;) {
						bool any = false;
						for (int t = 0; t < TILE * TILE * TILE; t++) {
							const int slot = (t % TILE + 1) + HALO * ((t / TILE) % TILE + 1) + HALO * HALO * (t / (TILE * TILE) + 1);
							ch[t] = flood_step(st, slot);
							any = any || ch[t];
						}
						for (int t = 0; t < TILE * TILE * TILE; t++)
							if (ch[t]) {
								const int lx = t % TILE, ly = (t / TILE) % TILE, lz = t / (TILE * TILE);
								st[(lx + 1) + HALO * (ly + 1) + HALO * HALO * (lz + 1)] = 2;
								next[(int64_t)(ox + lx) + d.Y * (oy + ly) + d.Z * (oz + lz)] = c;
								changed = true;
							}
						if (!any) break;
					}
					changedTiles += changed;
				}
		memcpy(phi, next, d.n * sizeof(float));
		if (!changedTiles) break;
	}
	free(st); free(ch); free(next);
	return rounds;
}

int main(int argc, char** argv) {
	if (argc < 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	int32_t h[6];
	float f[5];
	if (fread(h, 4, 6, in) != 6 || fread(f, 4, 5, in) != 5) return 2;
	Dim d;
	d.sx = h[0]; d.sy = h[1]; d.sz = h[2];
	d.is3d = 1; d.zoff = 0; d.gsz = d.sz;
	d.Y = d.sx; d.Z = (int64_t)d.sx * d.sy; d.n = d.Z * d.sz;
	const int64_t nNodes = h[3], nTris = h[4], n = d.n;
	const Params P = make_params(f[3], f[4]);
	float* pos = exact<float>(3 * nNodes);
	int32_t* tri = exact<int32_t>(3 * nTris);
	if (fread(pos, 4, 3 * nNodes, in) != (size_t)(3 * nNodes) || fread(tri, 4, 3 * nTris, in) != (size_t)(3 * nTris)) return 2;
	float* phi = exact<float>(n);
	if (h[5]) {
		if (fread(phi, 4, n, in) != (size_t)n) return 2;
		const int64_t counts[3] = {0, 0, flood(d, phi, P.cutoff)};
		fwrite(counts, 8, 3, out);
		fwrite(phi, 4, n, out);
		fclose(in); fclose(out);
		free(pos); free(tri); free(phi);
		return 0;
	}
	// sources: count, scan, emit
	const TriView T = {nTris, nTris, nNodes, nNodes, tri, pos};
	int64_t* off = exact<int64_t>(nTris);
	int64_t total = 0;
	for (int64_t t = 0; t < nTris; t++) {
		V3 p[3];
		if (!tri_nodes(T, t, p)) return 3;
		const Plan pl = tri_plan(p);
		if (pl.wrap) return 4;
		int64_t c = 1;
		for (int s0 = 0; s0 < pl.iterA; s0++) c += row_count(pl, s0);
		off[t] = total;
		total += c;
	}
	float *spos = exact<float>(3 * total), *snrm = exact<float>(3 * total), *bpos = exact<float>(3 * total), *bnrm = exact<float>(3 * total);
	const SrcOut S = {total, total, spos, snrm, f[0], f[1], f[2]};
	for (int64_t t = 0; t < nTris; t++) {
		V3 p[3];
		tri_nodes(T, t, p);
		const Plan pl = tri_plan(p);
		const V3 nrm = face_normal(p);
		int64_t o = off[t];
		put_source(S, o++, face_centre(p, S), nrm);
		for (int s0 = 0; s0 < pl.iterA; s0++) o = emit_row(pl, p, nrm, s0, o, S);
		if (o != (t + 1 < nTris ? off[t + 1] : total)) return 5;
	}
	// binning: counts, scan, stable placement
	const int64_t nocc = (int64_t)occ_dim(d.sx) * occ_dim(d.sy) * occ_dim(d.sz);
	int32_t *len = exact<int32_t>(n), *start = exact<int32_t>(n), *cur = exact<int32_t>(n), *occ = exact<int32_t>(nocc);
	for (int64_t s = 0; s < total; s++) {
		const int64_t c = cell_index(d, spos[s], spos[total + s], spos[2 * total + s]);
		if (c < 0) continue;
		len[c]++;
		occ[occ_index(d, (int)spos[s], (int)spos[total + s], (int)spos[2 * total + s])] = 1;
	}
	int64_t binned = 0;
	for (int64_t c = 0; c < n; c++) {
		start[c] = (int32_t)binned;
		binned += len[c];
	}
	for (int64_t s = 0; s < total; s++) {
		const int64_t c = cell_index(d, spos[s], spos[total + s], spos[2 * total + s]);
		if (c < 0) continue;
		const int64_t o = start[c] + cur[c]++;
		for (int q = 0; q < 3; q++) {
			bpos[q * total + o] = spos[q * total + s];
			bnrm[q * total + o] = snrm[q * total + s];
		}
	}
	// gather, flood
	const Gather G = {bpos, bnrm, total, len, start, occ, P};
	float* pre = exact<float>(n);
	for (int k = 0; k < d.sz; k++)
		for (int j = 0; j < d.sy; j++)
			for (int i = 0; i < d.sx; i++) pre[i + d.Y * j + d.Z * k] = gather_cell(d, G, i, j, k);
	memcpy(phi, pre, n * sizeof(float));
	const int64_t counts[3] = {total, binned, flood(d, phi, P.cutoff)};
	fwrite(counts, 8, 3, out);
	fwrite(spos, 4, 3 * total, out); fwrite(snrm, 4, 3 * total, out);
	fwrite(len, 4, n, out); fwrite(start, 4, n, out);
	fwrite(bpos, 4, 3 * total, out); fwrite(bnrm, 4, 3 * total, out);
	fwrite(pre, 4, n, out); fwrite(phi, 4, n, out);
	fclose(in); fclose(out);
	free(pos); free(tri); free(phi); free(off); free(spos); free(snrm); free(bpos); free(bnrm);
	free(len); free(start); free(cur); free(occ); free(pre);
	return 0;
}
