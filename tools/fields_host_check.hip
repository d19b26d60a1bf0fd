// tools/fields_host_check.hip -- the per-cell bodies of mantaflow_amd/csrc/fields_cells.h run on the HOST: every launch of fields.hip
// replaced by a serial loop over the cells, as a stand-alone program for the host sanitizers.  tools/fields_host_check.py drives it with
// the inputs of tests/fields_model.py and compares every output with the model bit for bit.  It makes no HIP call and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/fields_host_check.hip -o <scratch>/fields_host_check
//   python tools/fields_host_check.py <scratch>/fields_host_check
//
// usage: fields_host_check <op> <sx> <sy> <sz> <in.bin> <out.bin> [numbers...]; arrays are raw 4-byte words, Vec3 grids as 3 planes.
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/fields_cells.h"
#include <stdlib.h>
#include <string>
#include <vector>

using namespace mf;
using namespace mf::fields;

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

// exact-size heap arrays read from / written to the files in order
struct Io {
	FILE *in, *out;
	std::vector<float*> owned;
	float* take(int64_t words) {
		float* p = (float*)malloc(words * 4);
		if (fread(p, 4, words, in) != (size_t)words) { fprintf(stderr, "short input\n"); exit(2); }
		owned.push_back(p);
		return p;
	}
	void give(const void* p, int64_t words) { fwrite(p, 4, words, out); }
	~Io() {
		for (float* p : owned) free(p);
		fclose(in);
		fclose(out);
	}
};

#define FOR_CELLS(d)                                   \
	for (int k = 0; k < (d).sz; k++)                   \
		for (int j = 0; j < (d).sy; j++)               \
			for (int i = 0; i < (d).sx; i++) {         \
				const int64_t idx = i + (d).Y * j + (int64_t)(d).sx * (d).sy * k;
#define END_CELLS }

int main(int argc, char** argv) {
	if (argc < 7) return 2;
	const std::string op = argv[1];
	const Dim d = make_dim(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
	Io io;
	io.in = fopen(argv[5], "rb");
	io.out = fopen(argv[6], "wb");
	if (!io.in || !io.out) return 2;
	auto num = [&](int q) { return atof(argv[7 + q]); };
	const int64_t n = d.n;
	if (op == "burn") {
		const int present = atoi(argv[7]);       // bit q: optional grid q (red, green, blue, heat) is given
		float *fuel = io.take(n), *density = io.take(n), *react = io.take(n), *opt[4];
		for (int q = 0; q < 4; q++) opt[q] = (present >> q & 1) ? io.take(n) : nullptr;
		const Burn B = {(float)num(1), (float)num(2), (float)num(3), (float)num(4), (float)num(5), (float)num(6), (float)num(7), (float)num(8)};
		FOR_CELLS(d)
			if (interior(d, i, j, k)) process_burn(idx, fuel, density, react, opt[0], opt[1], opt[2], opt[3], B);
		END_CELLS
		io.give(fuel, n); io.give(density, n); io.give(react, n);
		for (int q = 0; q < 4; q++) if (opt[q]) io.give(opt[q], n);
	} else if (op == "flame") {
		float *react = io.take(n), *flame = io.take(n);
		FOR_CELLS(d)
			if (interior(d, i, j, k)) flame[idx] = update_flame(react[idx]);
		END_CELLS
		io.give(flame, n);
	} else if (op == "secderiv") {
		float *v = io.take(n), *ret = io.take(n);
		FOR_CELLS(d)
			if (interior(d, i, j, k)) ret[idx] = (float)five_point(d, v, idx);
		END_CELLS
		io.give(ret, n);
	} else if (op == "wave") {
		float *A0 = io.take(n), *Ai = io.take(n), *Aj = io.take(n), *Ak = io.take(n), *ut = io.take(n), *utm1 = io.take(n);
		float* rhs = (float*)malloc(n * 4);
		io.owned.push_back(rhs);
		FOR_CELLS(d)
			wave_system(d, idx, interior(d, i, j, k), A0, Ai, Aj, Ak, rhs, ut, utm1, (float)num(0), atoi(argv[8]));
		END_CELLS
		io.give(A0, n); io.give(Ai, n); io.give(Aj, n); io.give(Ak, n); io.give(rhs, n);
	} else if (op == "extrap") {
		const int ncomp = atoi(argv[7]), isInt = atoi(argv[8]), distance = atoi(argv[9]), flagFrom = atoi(argv[10]), flagTo = atoi(argv[11]);
		int32_t* flags = (int32_t*)io.take(n);
		float* val = io.take(ncomp * n);
		int32_t* tmp = (int32_t*)malloc(n * 4);
		io.owned.push_back((float*)tmp);
		for (int64_t q = 0; q < n; q++) tmp[q] = (flags[q] & flagFrom) ? 1 : 0;
		for (int dist = 1; dist <= distance; dist++) {
			FOR_CELLS(d)
				if (!interior(d, i, j, k)) continue;
				if (isInt) extrapolate_cell<int32_t>(d, idx, flags, tmp, (int32_t*)val, 1, dist, flagTo);
				else extrapolate_cell<float>(d, idx, flags, tmp, val, ncomp, dist, flagTo);
			END_CELLS
		}
		io.give(val, ncomp * n);
	} else {
		return 2;
	}
	return 0;
}
