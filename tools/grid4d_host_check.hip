// tools/grid4d_host_check.hip -- the per-cell bodies of mantaflow_amd/csrc/grid4d_cells.h run on the HOST: every launch of grid4d.hip
// replaced by a serial loop over the cells, as a stand-alone program for the host sanitizers.  tools/grid4d_host_check.py drives it with
// the inputs of tests/grid4d_model.py and compares every output with the model bit for bit.  It makes no HIP call and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/grid4d_host_check.hip -o <scratch>/grid4d_host_check
//   python tools/grid4d_host_check.py <scratch>/grid4d_host_check
//
// usage: grid4d_host_check <op> <sx> <sy> <sz> <st> <in.bin> <out.bin> [numbers...]; arrays are raw 4-byte words, the vector types as
// component planes.  Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/grid4d_cells.h"
#include <stdlib.h>
#include <string>
#include <vector>

using namespace mf;
using namespace mf::grid4d;

struct Io {
	FILE *in, *out;
	std::vector<void*> owned;
	void* fresh(int64_t words) {
		void* p = malloc(words * 4);
		owned.push_back(p);
		return p;
	}
	float* take(int64_t words) {
		float* p = (float*)fresh(words);
		if (fread(p, 4, words, in) != (size_t)words) { fprintf(stderr, "short input\n"); exit(2); }
		return p;
	}
	void give(const void* p, int64_t words) { fwrite(p, 4, words, out); }
	~Io() {
		for (void* p : owned) free(p);
		fclose(in);
		fclose(out);
	}
};

int main(int argc, char** argv) {
	if (argc < 8) return 2;
	const std::string op = argv[1];
	const Dim4 d = mkdim4(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
	Io io;
	io.in = fopen(argv[6], "rb");
	io.out = fopen(argv[7], "wb");
	if (!io.in || !io.out) return 2;
	auto num = [&](int q) { return atof(argv[8 + q]); };
	auto inum = [&](int q) { return atoi(argv[8 + q]); };
	const int64_t n = d.n;
	if (op == "bound") {            // ncomp w v0..v3 (words)
		const int ncomp = inum(0), w = inum(1);
		int32_t* g = (int32_t*)io.take(ncomp * n);
		for (int c = 0; c < ncomp; c++)
			for (int64_t idx = 0; idx < n; idx++)
				if (is_bound(d, cell_of(d, idx), w)) g[c * n + idx] = (int32_t)atoll(argv[10 + c]);
		io.give(g, ncomp * n);
	} else if (op == "neumann") {   // ncomp w; in place, as the kernel
		const int ncomp = inum(0), w = inum(1);
		int32_t* g = (int32_t*)io.take(ncomp * n);
		for (int c = 0; c < ncomp; c++)
			for (int64_t idx = 0; idx < n; idx++) {
				const int64_t src = neumann_source(d, cell_of(d, idx), w);
				if (src >= 0) g[c * n + idx] = g[c * n + src];
			}
		io.give(g, ncomp * n);
	} else if (op == "region") {    // ncomp start[4] end[4] value[4]
		const int ncomp = inum(0);
		float s[4], e[4], v[4];
		for (int q = 0; q < 4; q++) { s[q] = (float)num(1 + q); e[q] = (float)num(5 + q); v[q] = (float)num(9 + q); }
		float* g = io.take(ncomp * n);
		for (int c = 0; c < ncomp; c++)
			for (int64_t idx = 0; idx < n; idx++)
				if (in_region(cell_of(d, idx), s, e)) g[c * n + idx] = v[c];
		io.give(g, ncomp * n);
	} else if (op == "slice") {     // ncomp srct dx dy dz withT; the entry's range test on srct is repeated here
		const int ncomp = inum(0), srct = inum(1), dx = inum(2), dy = inum(3), dz = inum(4), withT = inum(5);
		const int64_t dn = (int64_t)dx * dy * dz;
		const int nd = ncomp == 4 ? 3 : 1;
		float* src = io.take(ncomp * n);
		float* dst = io.take(nd * dn);
		float* dstt = withT ? io.take(dn) : nullptr;
		if (srct >= 0 && srct < d.st)
			for (int c = 0; c < ncomp; c++)
				for (int64_t idx = 0; idx < d.T; idx++) {
					const int64_t di = slice_target(cell_of(d, idx), dx, dy, dz);
					if (di < 0) continue;
					const float val = src[c * n + d.T * srct + idx];
					if (c < 3) dst[c * dn + di] = val;
					else if (dstt) dstt[di] = val;
				}
		io.give(dst, nd * dn);
		if (dstt) io.give(dstt, dn);
	} else if (op == "interp") {    // ncomp tx ty tz tt fac[4] off[4]; d is the source
		const int ncomp = inum(0);
		const Dim4 td = mkdim4(inum(1), inum(2), inum(3), inum(4));
		float fac[4], off[4];
		for (int q = 0; q < 4; q++) { fac[q] = (float)num(5 + q); off[q] = (float)num(9 + q); }
		float* src = io.take(ncomp * n);
		float* dst = (float*)io.fresh(ncomp * td.n);
		for (int c = 0; c < ncomp; c++)
			for (int64_t idx = 0; idx < td.n; idx++) dst[c * td.n + idx] = interpolate_cell(d, src + c * n, cell_of(td, idx), fac, off);
		io.give(dst, ncomp * td.n);
	} else if (op == "norm") {      // ncomp -> min, max normSquare
		const int ncomp = inum(0);
		float* a = io.take(ncomp * n);
		float lo = FLT_MAX, hi = -FLT_MAX;
		for (int64_t idx = 0; idx < n; idx++) {
			const float s = norm_square(a, n, idx, ncomp);
			lo = fminf(lo, s);
			hi = fmaxf(hi, s);
		}
		io.give(&lo, 1);
		io.give(&hi, 1);
	} else if (op == "maxdiff") {   // ncomp isInt -> double (2 words)
		const int ncomp = inum(0), isInt = inum(1);
		float *a = io.take(ncomp * n), *b = io.take(ncomp * n);
		double m = 0.;
		for (int64_t idx = 0; idx < n; idx++) m = fmax(m, cell_diff(a, b, n, idx, ncomp, isInt));
		io.give(&m, 2);
	} else if (op == "int") {       // which v lo hi: 0 add 1 sub 2 mult 3 scaled add (factor v) 4 addConst 5 multConst 6 clamp
		const int which = inum(0), v = inum(1), lo = inum(2), hi = inum(3);
		int32_t *a = (int32_t*)io.take(n), *b = (int32_t*)io.take(n);
		for (int64_t idx = 0; idx < n; idx++) {
			const int32_t x = a[idx], y = b[idx];
			a[idx] = which == 0 ? add_i(x, y) : which == 1 ? sub_i(x, y) : which == 2 ? mul_i(x, y) : which == 3 ? add_i(x, mul_i(v, y))
			       : which == 4 ? add_i(x, v) : which == 5 ? mul_i(x, v) : clamp_i(x, lo, hi);
		}
		io.give(a, n);
	} else if (op == "pdside") {    // side isInt ncomp stride v(word): n = sx live slots of channels `stride` apart
		const int side = inum(0), isInt = inum(1), ncomp = inum(2);
		const int64_t np = d.sx, stride = inum(3);
		const int32_t v = (int32_t)atoll(argv[12]);
		int32_t* a = (int32_t*)io.take(ncomp * stride);
		float fv;
		memcpy(&fv, &v, 4);
		for (int c = 0; c < ncomp; c++)
			for (int64_t idx = 0; idx < np; idx++) {
				int32_t* p = a + c * stride + idx;
				if (isInt) *p = clamp_side<int32_t>(side, v, *p);
				else *(float*)p = clamp_side<float>(side, fv, *(float*)p);
			}
		io.give(a, ncomp * stride);
	} else if (op == "pdterms") {   // what isInt ncomp stride -> the term of every live slot (component 0 for what 0), as doubles
		const int what = inum(0), isInt = inum(1), ncomp = inum(2);
		const int64_t np = d.sx, stride = inum(3);
		float* a = io.take(ncomp * stride);
		for (int64_t idx = 0; idx < np; idx++) {
			const double term = sum_term(what, isInt, ncomp, 0, a, stride, idx);
			io.give(&term, 2);
		}
	} else if (op == "sym") {       // mac withErr symmetrize axis bound disable: d.sx, d.sy, d.sz are a 3-D grid (st == 1), as the entry sweeps it
		const int mac = inum(0), withErr = inum(1), symm = inum(2), axis = inum(3), bound = inum(4), disable = inum(5);
		Dim g;
		g.sx = d.sx; g.sy = d.sy; g.sz = d.sz;
		g.is3d = d.sz > 1;
		g.zoff = 0; g.gsz = d.sz;
		g.Y = d.sx; g.Z = g.is3d ? (int64_t)d.sx * d.sy : 0; g.n = (int64_t)d.sx * d.sy * d.sz;
		float* a = io.take((mac ? 3 : 1) * g.n);
		float* err = withErr ? io.take(g.n) : nullptr;
		if (mac && err) for (int64_t q = 0; q < g.n; q++) err[q] = 0.f;
		for (int q = 0; q < (mac ? 3 : 1); q++) {
			if (mac && (disable >> q & 1)) continue;
			const Sym S = {axis, bound, symm, mac && q == 0};
			for (int pass = 0; pass < 2; pass++)
				for (int k = 0; k < g.sz; k++)
					for (int j = 0; j < g.sy; j++)
						for (int i = 0; i < g.sx; i++) sym_cell(g, i, j, k, pass, S, a + (mac ? (axis + q) % 3 : 0) * g.n, err, mac != 0);
		}
		io.give(a, (mac ? 3 : 1) * g.n);
		if (err) io.give(err, g.n);
	} else if (op == "safediv") {
		int32_t *a = (int32_t*)io.take(n), *b = (int32_t*)io.take(n);
		for (int64_t idx = 0; idx < n; idx++) a[idx] = safe_div_i(a[idx], b[idx]);
		io.give(a, n);
	} else {
		return 2;
	}
	return 0;
}
