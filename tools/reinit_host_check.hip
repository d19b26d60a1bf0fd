// tools/reinit_host_check.hip -- the bodies of mantaflow_amd/csrc/reinit_cells.h run on the HOST: every launch of reinit.hip replaced by a
// serial loop (the seeding by a loop over the cells, the min-reduction by a loop over the list, a sub-round by a selecting loop followed
// by a popping loop), next to the literal serial march, as a stand-alone program for the host sanitizers.  tools/reinit_host_check.py
// drives it with every fixture case of tests/reinit_model.py and compares both with the model.  It makes no HIP call and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/reinit_host_check.hip -o <scratch>/reinit_host_check
//   python tools/reinit_host_check.py <scratch>/reinit_host_check
//
// usage: reinit_host_check <in.bin> <out.bin>
//   in:  int32 sx, sy, sz, hasVel, ignoreWalls, correctOuterLayer, obstacleType; float maxTime; phi[n]; flags[n]; (hasVel: vel[3][n])
//   out: twice (the serial call, then the call in rounds): phi[n], (hasVel: vel[3][n]), fmFlags[n], keys[n];
//        then int64 serial pops[2], and windows[2], sub-rounds[2], pops[2], serial[2] of the call in rounds
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/reinit_cells.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace mf;
using namespace mf::reinit;

static Dim make_dim(int sx, int sy, int sz) {
	Dim d;
	d.sx = sx; d.sy = sy; d.sz = sz;
	d.is3d = sz > 1;
	d.zoff = 0; d.gsz = sz;
	d.Y = sx;
	d.Z = d.is3d ? (int64_t)sx * sy : 0;
	d.n = (int64_t)sx * sy * sz;
	return d;
}

template <class T>
static T* exact(int64_t count) { return (T*)calloc(count ? count : 1, sizeof(T)); }

struct Stats {
	int64_t windows[2], subrounds[2], pops[2], serial[2];
};

static void rounds_march(March m, bool outer, float* snapPhi, int32_t* snapFm, float* snapVel, int32_t* list, int32_t* sel, int32_t* epoch,
                         Stats& S) {
	m.epoch = epoch;
	const Dim& d = m.d;
	const int s = m.dir > 0;
	for (int64_t idx = 0; idx < d.n; idx++) {
		int i, j, k;
		cell_ijk(d, idx, i, j, k);
		init_fm(m, idx, i, j, k);
	}
	memcpy(snapPhi, m.phi, d.n * sizeof(float));
	memcpy(snapFm, m.fm, d.n * sizeof(int32_t));
	if (m.vel) memcpy(snapVel, m.vel, 3 * d.n * sizeof(float));
	m.fm0 = snapFm;
	int64_t count = 0;
	for (int64_t idx = 0; idx < d.n; idx++) {
		int i, j, k;
		cell_ijk(d, idx, i, j, k);
		if (outer ? seed_outer(m, idx, i, j, k) : seed_interface(m, idx, i, j, k)) list[count++] = (int32_t)idx;
	}
	bool flag = false;
	int w = 0;
	while (!flag) {
		int64_t live = 0;
		float T = 0.f;
		for (int64_t e = 0; e < count; e++) {
			const int64_t c = list[e];
			if (m.fm[c] != FM_ONHEAP) continue;
			if (!live || (m.dir > 0 ? m.key[c] < T : m.key[c] > T)) T = m.key[c];
			live++;
		}
		if (!live) break;
		const float te = window_end(m.dir, T);
		S.windows[s]++;
		w++;
		for (;;) {
			int64_t nW = 0, nSel = 0, joined = 0;
			for (int64_t e = 0; e < count; e++) {
				const int64_t c = list[e];
				if (m.fm[c] != FM_ONHEAP || !in_window(m.dir, m.key[c], te)) continue;
				nW++;
				if (selectable(m, c, te)) sel[nSel++] = (int32_t)c;
			}
			for (int64_t e = 0; e < nSel; e++) m.epoch[sel[e]] = w;
			if (nW == 0 || nSel == 0) {
				flag = true;
				break;
			}
			S.subrounds[s]++;
			S.pops[s] += nSel;
			for (int64_t e = 0; e < nSel; e++)
				pop_cell(m, sel[e], [&](int64_t q) {
					list[count++] = (int32_t)q;
					if (in_window(m.dir, m.key[q], te)) joined++;
					if (late_conflict(m, q, w)) flag = true;
				});
			if (flag || (nSel == nW && joined == 0)) break;
		}
	}
	if (flag) {
		memcpy(m.phi, snapPhi, d.n * sizeof(float));
		memcpy(m.fm, snapFm, d.n * sizeof(int32_t));
		if (m.vel) memcpy(m.vel, snapVel, 3 * d.n * sizeof(float));
		memset(m.key, 0, d.n * sizeof(float));
		S.windows[s] = S.subrounds[s] = 0;
		S.serial[s] = 1;
		m.epoch = nullptr;
		S.pops[s] = serial_march(m, outer);
		return;
	}
	for (int64_t idx = 0; idx < d.n; idx++) {
		int i, j, k;
		cell_ijk(d, idx, i, j, k);
		snapPhi[idx] = boundary_value(d, m.phi, i, j, k);
	}
	memcpy(m.phi, snapPhi, d.n * sizeof(float));
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[7];
	float maxTime;
	if (fread(h, 4, 7, f) != 7 || fread(&maxTime, 4, 1, f) != 1) return 2;
	const Dim d = make_dim(h[0], h[1], h[2]);
	const int hasVel = h[3], ignoreWalls = h[4], outer = h[5], obsType = h[6];
	float* phi0 = exact<float>(d.n);
	int32_t* flags = exact<int32_t>(d.n);
	float* vel0 = exact<float>(hasVel ? 3 * d.n : 0);
	if ((int64_t)fread(phi0, 4, d.n, f) != d.n || (int64_t)fread(flags, 4, d.n, f) != d.n) return 2;
	if (hasVel && (int64_t)fread(vel0, 4, 3 * d.n, f) != 3 * d.n) return 2;
	fclose(f);
	FILE* o = fopen(argv[2], "wb");
	if (!o) return 2;
	float *phi = exact<float>(d.n), *key = exact<float>(d.n), *vel = exact<float>(hasVel ? 3 * d.n : 0);
	int32_t* fm = exact<int32_t>(d.n);
	auto emit = [&]() {
		fwrite(phi, 4, d.n, o);
		if (hasVel) fwrite(vel, 4, 3 * d.n, o);
		fwrite(fm, 4, d.n, o);
		fwrite(key, 4, d.n, o);
	};
	auto start = [&]() {
		memcpy(phi, phi0, d.n * sizeof(float));
		if (hasVel) memcpy(vel, vel0, 3 * d.n * sizeof(float));
		memset(fm, 0xff, d.n * sizeof(int32_t));         // scratch arrives dirty
		memset(key, 0xff, d.n * sizeof(float));
	};
	int64_t spops[2] = {0, 0};
	start();
	serial_call(d, phi, fm, key, flags, hasVel ? vel : nullptr, maxTime, ignoreWalls, outer, obsType, spops);
	emit();
	start();
	Stats S;
	memset(&S, 0, sizeof(S));
	float *snapPhi = exact<float>(d.n), *snapVel = exact<float>(hasVel ? 3 * d.n : 0);
	int32_t *snapFm = exact<int32_t>(d.n), *list = exact<int32_t>(d.n), *sel = exact<int32_t>(d.n), *epoch = exact<int32_t>(d.n);
	memset(epoch, 0xff, d.n * sizeof(int32_t));
	for (int dir = -1; dir <= 1; dir += 2) {
		const March m = {d, phi, fm, key, fm, flags, dir > 0 && hasVel ? vel : nullptr, maxTime * (float)dir, dir, ignoreWalls, obsType, nullptr};
		rounds_march(m, dir > 0 && outer, snapPhi, snapFm, snapVel, list, sel, epoch, S);
		const float val = dir < 0 ? (float)(-(double)maxTime - 1.) : (float)((double)maxTime + 1.);
		for (int64_t idx = 0; idx < d.n; idx++) {
			int i, j, k;
			cell_ijk(d, idx, i, j, k);
			set_uninitialized(m, idx, i, j, k, val);
		}
	}
	emit();
	fwrite(spops, 8, 2, o);
	fwrite(&S, sizeof(S), 1, o);
	fclose(o);
	free(phi0); free(flags); free(vel0); free(phi); free(key); free(vel); free(fm);
	free(snapPhi); free(snapVel); free(snapFm); free(list); free(sel); free(epoch);
	return 0;
}
