// tools/mg2d_host_check.hip -- the per-vertex bodies of mantaflow_amd/csrc/mg2d_cells.h (and set_rhs, ordered_sum of mg_host.h) run on the
// HOST: every launch that mg_driver.h makes for the 2-D hierarchy of mg2d.hip
// replaced by a serial loop over its work items (in the stride-1 form the grid-wide kernels use and, for the levels of the tail, in
// the stride-1024 form of the single-workgroup kernel), the tail's coarsest-level CG by a serial loop over the same per-vertex
// steps, as a stand-alone program for the host sanitizers.  tools/mg2d_host_check.py drives it with the cases of
// tests/mg2d_cases.py and compares every output with the numpy model and the recorded paths bit for bit.  It makes no HIP call and
// needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/mg2d_host_check.hip -o <scratch>/mg2d_host_check
//   python tools/mg2d_host_check.py <scratch>/mg2d_host_check
//
// usage: mg2d_host_check <in.bin> <out.bin> <tail_verts>
//   in:  int32 sx, sy; float accuracy; float A0[n], Ai[n], Aj[n], rhs[n]
//   out: int32 nl, tail_first, cg_iterations, info1, info2, npaths; int32 paths[npaths][12] (the layout of tools/mg2d_record.cpp);
//        per level: int32 sx, sy, active; uint8 t[n]; float A[3 or 5][n]; float b[n]; float x[n]
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.  x, b and r start as
// NaN: a pass that reads what no pass wrote shows in the comparison.
#include "../mantaflow_amd/csrc/mg2d_cells.h"
#include <math.h>
#include <stdlib.h>
#include <vector>

using namespace mf;
using namespace mf::mg2d;

template <class T>
static T* exact(int64_t count) { return (T*)calloc(count ? count : 1, sizeof(T)); }

static float* nans(int n) {
	float* p = exact<float>(n);
	for (int i = 0; i < n; i++) p[i] = NAN;
	return p;
}

// the tail's solveCG (k_mg_tail of mg_driver.h), stated a second time and serially, one vertex after the other: the same per-vertex steps between the same barriers
static int solve_cg(const Lv& L, bool l0, float accuracy) {
	const int n = L.n;
	double *x = exact<double>(n), *r = exact<double>(n), *z = exact<double>(n), *p = exact<double>(n), *s1 = exact<double>(n), *s2 = exact<double>(n);
	for (int v = 0; v < n; v++) x[v] = (double)L.x[v];
	for (int v = 0; v < n; v++) {
		if (L.t[v] == vtInactive) continue;
		r[v] = L.b[v] - cg_apply(L, l0, v, v % L.sx, v / L.sx, x);
		z[v] = r[v] / L.A[v];
		p[v] = z[v];
		s1[v] = r[v] * r[v];
		s2[v] = r[v] * z[v];
	}
	const double initialResidual = sqrt(ordered_sum(s1, n));
	double alphaTop = ordered_sum(s2, n);
	int iter = 0;
	for (; iter < 10000 && initialResidual > 1E-12; iter++) {
		for (int v = 0; v < n; v++) {
			s1[v] = 0.0;
			if (L.t[v] == vtInactive) continue;
			z[v] = cg_apply(L, l0, v, v % L.sx, v / L.sx, p);
			s1[v] = p[v] * z[v];
		}
		const double alpha = alphaTop / ordered_sum(s1, n);
		for (int v = 0; v < n; v++) {
			s1[v] = s2[v] = 0.0;
			if (L.t[v] == vtInactive) continue;
			x[v] += alpha * p[v];
			r[v] -= alpha * z[v];
			z[v] = r[v] / L.A[v];
			s1[v] = r[v] * r[v];
			s2[v] = r[v] * z[v];
		}
		const double residual = sqrt(ordered_sum(s1, n));
		const double alphaTopNew = ordered_sum(s2, n);
		if (residual / initialResidual < accuracy) break;
		const double beta = alphaTopNew / alphaTop;
		alphaTop = alphaTopNew;
		for (int v = 0; v < n; v++) p[v] = z[v] + beta * p[v];
	}
	for (int v = 0; v < n; v++) L.x[v] = (float)x[v];
	free(x); free(r); free(z); free(p); free(s1); free(s2);
	return iter;
}

// a pass as `workers` workers that stride by `workers`, one worker after the other (1: the whole range by one worker)
template <class F>
static void run(int workers, F pass) {
	for (int w = 0; w < workers; w++) pass(w, workers);
}

int main(int argc, char** argv) {
	if (argc != 4) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 3;
	int32_t hdr[2];
	float accuracy;
	if (fread(hdr, 4, 2, f) != 2 || fread(&accuracy, 4, 1, f) != 1) return 3;
	const int sx = hdr[0], sy = hdr[1], n0 = sx * sy;
	const int tail_verts = atoi(argv[3]);
	float *A0 = exact<float>(n0), *Ai = exact<float>(n0), *Aj = exact<float>(n0), *rhs = exact<float>(n0);
	if ((int)fread(A0, 4, n0, f) != n0 || (int)fread(Ai, 4, n0, f) != n0 || (int)fread(Aj, 4, n0, f) != n0 || (int)fread(rhs, 4, n0, f) != n0) return 3;
	fclose(f);

	View V;
	int sizes[MAXL][2];
	V.nl = pyramid(sx, sy, sizes);
	for (int l = 0; l < V.nl; l++) {
		Lv& L = V.l[l];
		L.sx = sizes[l][0];
		L.sy = sizes[l][1];
		L.n = L.sx * L.sy;
		L.A = exact<float>((int64_t)L.n * (l == 0 ? 3 : 5));
		L.x = nans(L.n);
		L.b = nans(L.n);
		L.r = nans(L.n);
		L.t = exact<unsigned char>(L.n);
	}
	int tail_first = V.nl - 1;
	while (tail_first > 0 && V.l[tail_first - 1].n <= tail_verts) tail_first--;

	// set-up (set_a of mg_driver.h)
	int info[3] = {0, 0, 0};
	int active[MAXL];
	const std::vector<Path> ps = make_paths();
	Path* paths = exact<Path>((int64_t)ps.size());
	for (size_t i = 0; i < ps.size(); i++) paths[i] = ps[i];
	for (int v = 0; v < n0; v++) copy_activate(V.l[0], v, A0, Ai, Aj, info);
	active[0] = 0;
	for (int v = 0; v < n0; v++) active[0] += V.l[0].t[v] != vtInactive;
	for (int l = 1; l < V.nl; l++) {
		active[l] = select_coarse(dim_of(V.l[l - 1]), V.l[l - 1].t, dim_of(V.l[l]), V.l[l].t);
		for (int idx = 0; idx < V.l[l].n; idx++) {
			if (l == 1) operator1(V.l[0], V.l[1], idx, paths, (int)ps.size());
			else operatorN(V.l[l - 1], V.l[l], idx);
		}
	}

	// one V-cycle (vcycle of mg_driver.h): grid-wide kernels above tail_first (stride = the whole grid: every item by its own thread), the tail's
	// 1024 workers below
	const int last = V.nl - 1;
	for (int v = 0; v < n0; v++) set_rhs(V.l[0], v, rhs);
	for (int l = 0; l < last; l++) {
		const Lv& L = V.l[l];
		const bool l0 = l == 0;
		const int workers = l < tail_first ? 1 : 1024;
		for (int c = 0; c < smooth_colours(l0); c++) run(workers, [&](int s, int st) { pass_smooth(L, l0, c, s, st); });
		run(workers, [&](int s, int st) { pass_residual(L, l0, s, st); });
		run(workers, [&](int s, int st) { pass_restrict(L, V.l[l + 1], s, st); });
	}
	const int cg_iters = solve_cg(V.l[last], last == 0, accuracy);
	for (int l = last - 1; l >= 0; l--) {
		const Lv& L = V.l[l];
		const bool l0 = l == 0;
		const int workers = l < tail_first ? 1 : 1024;
		run(workers, [&](int s, int st) { pass_interp_add(L, V.l[l + 1], s, st); });
		for (int c = smooth_colours(l0) - 1; c >= 0; c--) run(workers, [&](int s, int st) { pass_smooth(L, l0, c, s, st); });
	}

	f = fopen(argv[2], "wb");
	if (!f) return 4;
	const int32_t head[6] = {V.nl, tail_first, cg_iters, info[1], info[2], (int32_t)ps.size()};
	fwrite(head, 4, 6, f);
	for (const Path& p : ps) {
		int32_t o[12] = {p.N[0], p.N[1], p.U[0], p.U[1], p.W[0], p.W[1], p.sc, p.sf, p.inU, 0, 0, 0};
		memcpy(o + 9, &p.rw, 4);
		memcpy(o + 10, &p.iw, 4);
		fwrite(o, 4, 12, f);
	}
	for (int l = 0; l < V.nl; l++) {
		const Lv& L = V.l[l];
		const int32_t lh[3] = {L.sx, L.sy, active[l]};
		fwrite(lh, 4, 3, f);
		fwrite(L.t, 1, L.n, f);
		fwrite(L.A, 4, (size_t)L.n * (l == 0 ? 3 : 5), f);
		fwrite(L.b, 4, L.n, f);
		fwrite(L.x, 4, L.n, f);
	}
	fclose(f);
	for (int l = 0; l < V.nl; l++) {
		free(V.l[l].A); free(V.l[l].x); free(V.l[l].b); free(V.l[l].r); free(V.l[l].t);
	}
	free(paths); free(A0); free(Ai); free(Aj); free(rhs);
	return 0;
}
