// tools/vsheet_host_check.hip -- the per-element bodies of mantaflow_amd/csrc/vsheet_cells.h run on the HOST: every launch of vsheet.hip
// that calls them replaced by a serial loop, as a stand-alone program for the host sanitizers.  tools/vsheet_host_check.py drives it with
// the cases of tests/vsheet_model.py and compares every output with the model and the recorded reference bit for bit.  It makes no HIP
// call and needs no GPU.  (The shape test, the MAC sampler and the ordered inflow sum are device text of shape_inside.h and common.h and
// are not part of this program; the acceleration samples of vorticitySource are an input here.  The spreading runs its two bodies with
// every cell walking all triangles in ascending number: the binning and the merge of vsheet.hip are not host text.)
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/vsheet_host_check.hip -o <scratch>/vsheet_host_check
//   python tools/vsheet_host_check.py <scratch>/vsheet_host_check
//
// usage: vsheet_host_check <geometry|calc|source|weights|passes|spread> <in.bin> <out.bin> [arguments]
//   in:  int64 n, t; pos[3][n]; flags[n]; tri[3][t]; then per mode
//        calc:     circulation[3][t]                                   out: vorticity[3][t]
//        geometry: -                                                   out: centre[3][t]; area[t]; normal[3][t]; int32 fixed[t]
//        source:   vorticity[3][t]; a[3][t]; arguments hasVel gx gy gz scale maxAmount mult dt dx
//                                                                      out: vorticity[3][t]; v[t]
//        weights:  int32 opposite[3t]; argument mult                   out: weights[3t]; int32 index[3t]
//        passes:   weights[3t]; int32 index[3t]; vorticity[3][t]; arguments iter alpha
//                                                                      out: smoothed[3][t]
//        spread:   vorticity[3][t]; int32 flags[sx * sy * sz]; arguments sx sy sz sigma
//                                                                      out: wnorm[t]; vort[3][sx * sy * sz]
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/vsheet_cells.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

using namespace mf::vsheet;

template <class T>
static T* exact(int64_t count) { return (T*)calloc(count ? count : 1, sizeof(T)); }
template <class T>
static T* take(FILE* f, int64_t count) {
	T* a = exact<T>(count);
	if (count && fread(a, sizeof(T), count, f) != (size_t)count) {
		fprintf(stderr, "short input\n");
		exit(2);
	}
	return a;
}
template <class T>
static void put(FILE* f, const T* a, int64_t count) {
	if (count) fwrite(a, sizeof(T), count, f);
}

int main(int argc, char** argv) {
	if (argc < 4) return 2;
	const std::string mode = argv[1];
	FILE* in = fopen(argv[2], "rb");
	FILE* out = fopen(argv[3], "wb");
	if (!in || !out) return 2;
	int64_t nt[2];
	if (fread(nt, sizeof(int64_t), 2, in) != 2) return 2;
	const int64_t n = nt[0], t = nt[1];
	float* pos = take<float>(in, 3 * n);
	int32_t* flags = take<int32_t>(in, n);
	int32_t* tri = take<int32_t>(in, 3 * t);
	const MeshView M = {t, t, n, n, tri, pos, flags};
	for (int64_t i = 0; i < t; i++)
		if (tri_outside(M, i)) return 3;
	if (mode == "calc") {
		float* circ = take<float>(in, 3 * t);
		float* vort = exact<float>(3 * t);
		for (int64_t i = 0; i < t; i++) store3(vort, t, i, calc_vorticity(M, i, load3(circ, t, i)));
		put(out, vort, 3 * t);
		free(circ);
		free(vort);
	} else if (mode == "geometry") {
		float *c = exact<float>(3 * t), *area = exact<float>(t), *nrm = exact<float>(3 * t);
		int32_t* fixed = exact<int32_t>(t);
		for (int64_t i = 0; i < t; i++) {
			store3(c, t, i, face_center(M, i));
			area[i] = face_area(M, i);
			store3(nrm, t, i, face_normal(M, i));
			fixed[i] = tri_fixed(M, i);
		}
		put(out, c, 3 * t);
		put(out, area, t);
		put(out, nrm, 3 * t);
		put(out, fixed, t);
		free(c);
		free(area);
		free(nrm);
		free(fixed);
	} else if (mode == "source" && argc == 13) {
		float *vort = take<float>(in, 3 * t), *a = take<float>(in, 3 * t), *v = exact<float>(t);
		const int hasVel = atoi(argv[4]);
		float p[8];
		for (int q = 0; q < 8; q++) p[q] = strtof(argv[5 + q], nullptr);
		for (int64_t i = 0; i < t; i++) {
			V3 w = load3(vort, t, i);
			v[i] = vorticity_source(M, i, hasVel, load3(a, t, i), V3{p[0], p[1], p[2]}, p[3], p[4], p[5], p[6], p[7], w);
			store3(vort, t, i, w);
		}
		put(out, vort, 3 * t);
		put(out, v, t);
		free(vort);
		free(a);
		free(v);
	} else if (mode == "weights" && argc == 5) {
		int32_t* opp = take<int32_t>(in, 3 * t);
		float* w = exact<float>(3 * t);
		int32_t* idx = exact<int32_t>(3 * t);
		const float mult = strtof(argv[4], nullptr);
		for (int64_t c = 0; c < 3 * t; c++) {
			if (opp[c] >= 3 * t) return 3;
			smooth_weight(M, opp, c / 3, (int)(c % 3), mult, w[c], idx[c]);
		}
		put(out, w, 3 * t);
		put(out, idx, 3 * t);
		free(opp);
		free(w);
		free(idx);
	} else if (mode == "passes" && argc == 6) {
		float* w = take<float>(in, 3 * t);
		int32_t* idx = take<int32_t>(in, 3 * t);
		float *a = take<float>(in, 3 * t), *b = exact<float>(3 * t);
		const int iter = atoi(argv[4]);
		const float alpha = strtof(argv[5], nullptr);
		for (int it = 0; it < iter; it++) {
			for (int64_t i = 0; i < t; i++) store3(b, t, i, smooth_pass(t, w, idx, a, i));
			float* s = a;
			a = b;
			b = s;
		}
		for (int64_t i = 0; i < t; i++) store3(b, t, i, load3(a, t, i) * alpha);
		put(out, b, 3 * t);
		free(w);
		free(idx);
		free(a);
		free(b);
	} else if (mode == "spread" && argc == 8) {
		const int sx = atoi(argv[4]), sy = atoi(argv[5]), sz = atoi(argv[6]);
		const float sigma = strtof(argv[7], nullptr);
		const int64_t cells = (int64_t)sx * sy * sz;
		float* vort = take<float>(in, 3 * t);
		int32_t* gf = take<int32_t>(in, cells);
		float *wn = exact<float>(t), *grid = exact<float>(3 * cells);
		const Spread S = {sx, sy, sz, (int)ceilf(sigma), sigma, (float)(M_PI / (double)sigma), gf};
		for (int64_t i = 0; i < t; i++) wn[i] = spread_wnorm(S, face_center(M, i));
		for (int64_t c = 0; c < cells; c++) {
			V3 acc = {0.f, 0.f, 0.f};
			if (gf[c] & 1)
				for (int64_t i = 0; i < t; i++)
					spread_add(S, face_center(M, i), (load3(vort, t, i) * face_area(M, i)) * 16.0f, wn[i], (int)(c % sx), (int)((c / sx) % sy), (int)(c / ((int64_t)sx * sy)), acc);
			store3(grid, cells, c, acc);
		}
		put(out, wn, t);
		put(out, grid, 3 * cells);
		free(vort);
		free(gf);
		free(wn);
		free(grid);
	} else {
		return 2;
	}
	free(pos);
	free(flags);
	free(tri);
	fclose(in);
	fclose(out);
	return 0;
}
