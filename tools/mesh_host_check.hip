// tools/mesh_host_check.hip -- the per-cell bodies of mantaflow_amd/csrc/mesh_cells.h run on the HOST: the classify, count and emit
// launches of mesh.hip replaced by serial loops over the cells and the two scans by serial sums, as a stand-alone program for the host
// sanitizers.  tools/mesh_host_check.py drives it with the createMesh cases of tests/mesh_model.py and compares every output with the
// model bit for bit.  It makes no HIP call and needs no GPU.  (The node advection interpolates through common.h's device-only
// interpol_mac and is not part of this program.)
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/mesh_host_check.hip -o <scratch>/mesh_host_check
//   python tools/mesh_host_check.py <scratch>/mesh_host_check
//
// usage: mesh_host_check <sx> <sy> <sz> <in.bin> <out.bin>; in: phi; out: int64 counts[2], pos[3][n], normal[3][n], flags[n], tri[3][t],
// tflags[t].  Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/mesh_cells.h"
#include <stdlib.h>

using namespace mf;
using namespace mf::mesh;

template <class T>
static T* exact(int64_t count) { return (T*)malloc(count ? count * sizeof(T) : 1); }

int main(int argc, char** argv) {
	if (argc < 6) return 2;
	Dim d;
	d.sx = atoi(argv[1]); d.sy = atoi(argv[2]); d.sz = atoi(argv[3]);
	if (d.sx < 3 || d.sy < 3 || d.sz < 3) return 2;
	d.is3d = 1; d.zoff = 0; d.gsz = d.sz;
	d.Y = d.sx; d.Z = (int64_t)d.sx * d.sy; d.n = d.Z * d.sz;
	FILE* in = fopen(argv[4], "rb");
	FILE* out = fopen(argv[5], "wb");
	if (!in || !out) return 2;
	const int64_t n = d.n;
	float* phi = exact<float>(n);
	if (fread(phi, 4, n, in) != (size_t)n) return 2;
	uint8_t* cube = exact<uint8_t>(n);
	uint16_t* mask = exact<uint16_t>(n);
	int32_t *nodeOff = exact<int32_t>(n), *triOff = exact<int32_t>(n);
#define FOR_CELLS                              \
	for (int k = 0; k < d.sz; k++)             \
		for (int j = 0; j < d.sy; j++)         \
			for (int i = 0; i < d.sx; i++) {   \
				const int64_t idx = i + d.Y * j + d.Z * k;
	FOR_CELLS
		cube[idx] = (uint8_t)classify_cell(d, phi, i, j, k);
	}
	FOR_CELLS
		const unsigned c = cube[idx];
		const unsigned m = c ? owned_mask(d, cube, i, j, k, c) : 0u;
		mask[idx] = (uint16_t)m;
		nodeOff[idx] = __builtin_popcount(m);
		triOff[idx] = c ? tri_count(c) : 0;
	}
	int64_t nn = 0, nt = 0;
	for (int64_t idx = 0; idx < n; idx++) {
		const int32_t a = nodeOff[idx], b = triOff[idx];
		nodeOff[idx] = (int32_t)nn;
		triOff[idx] = (int32_t)nt;
		nn += a;
		nt += b;
	}
	MeshOut M = {nn, nt, nn, nt, exact<float>(3 * nn), exact<float>(3 * nn), exact<int32_t>(nn), exact<int32_t>(3 * nt), exact<int32_t>(nt)};
	memset(M.pos, 0xff, 12 * nn); memset(M.normal, 0xff, 12 * nn); memset(M.nflags, 0xff, 4 * nn);
	memset(M.tri, 0xff, 12 * nt); memset(M.tflags, 0xff, 4 * nt);
	FOR_CELLS
		(void)idx;
		emit_cell(d, phi, cube, mask, nodeOff, triOff, i, j, k, M);
	}
	const int64_t counts[2] = {nn, nt};
	fwrite(counts, 8, 2, out);
	fwrite(M.pos, 4, 3 * nn, out); fwrite(M.normal, 4, 3 * nn, out); fwrite(M.nflags, 4, nn, out);
	fwrite(M.tri, 4, 3 * nt, out); fwrite(M.tflags, 4, nt, out);
	fclose(in); fclose(out);
	free(phi); free(cube); free(mask); free(nodeOff); free(triOff);
	free(M.pos); free(M.normal); free(M.nflags); free(M.tri); free(M.tflags);
	return 0;
}
