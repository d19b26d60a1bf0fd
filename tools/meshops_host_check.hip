// tools/meshops_host_check.hip -- the per-element bodies of mantaflow_amd/csrc/meshops_cells.h run on the HOST: every launch of
// meshops.hip replaced by a serial loop, the radix sorts by std::stable_sort on the same keys, the scans by serial sums and the
// labelling rounds by a serial minimum-label sweep, as a stand-alone program for the host sanitizers.  tools/meshops_host_check.py
// drives it with the cases of tests/meshops_model.py and compares every output with the model bit for bit.  It makes no HIP call and
// needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/meshops_host_check.hip -o <scratch>/meshops_host_check
//   python tools/meshops_host_check.py <scratch>/meshops_host_check
//
// usage: meshops_host_check <conn|smooth|kill> <in.bin> <out.bin> [str minLength steps | elements]
//   in:  int64 n, t; pos[3][n]; normal[3][n]; flags[n]; tri[3][t]; tflags[t]
//   out: conn:   int32 counts[4] (groups of one, of three or more, first repeated, first out of range); opposite[3t]; nodeOff[n+1];
//                int32 ringLen; ringNodes[ringLen]; triOff[n+1]; ringTris[3t]          (nothing after the counts when refused)
//        smooth: pos[3][n] after the steps (no rescale); double terms[4][t] of those positions
//        kill:   int64 n', t'; pos[3][n']; normal[3][n']; flags[n']; tri[3][t']; tflags[t']
// Every array is allocated at its exact size on the heap, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/meshops_cells.h"
#include <algorithm>
#include <limits.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace mf;
using namespace mf::meshops;

template <class T>
static T* exact(int64_t count) { return (T*)calloc(count ? count : 1, sizeof(T)); }

struct Conn {
	int32_t counts[4];
	int32_t *opposite, *nodeOff, *ringNodes, *triOff, *ringTris;
	int64_t ringLen;
};

// the stable sort of `val` by key(val), as one pass of the radix sort
template <class F>
static void sort_by(int32_t* val, int64_t m, F key) {
	std::stable_sort(val, val + m, [&](int32_t a, int32_t b) { return key(a) < key(b); });
}

static bool build(const Tris& T, Conn* C) {
	const int64_t n = 3 * T.nTris, m = 6 * T.nTris;
	C->counts[0] = C->counts[1] = 0;
	C->counts[2] = C->counts[3] = -1;
	for (int64_t t = T.nTris - 1; t >= 0; t--) {
		const int f = tri_fault(T, t);
		if (f) C->counts[f == 2 ? 2 : 3] = (int32_t)t;
	}
	C->opposite = exact<int32_t>(n);
	C->nodeOff = exact<int32_t>(T.nNodes + 1);
	C->triOff = exact<int32_t>(T.nNodes + 1);
	C->ringTris = exact<int32_t>(n);
	C->ringNodes = nullptr;
	C->ringLen = 0;
	if (C->counts[2] >= 0 || C->counts[3] >= 0) return false;
	int32_t* val = exact<int32_t>(m);
	for (int64_t c = 0; c < n; c++) val[c] = (int32_t)c;
	sort_by(val, n, [&](int32_t c) { int32_t lo, hi; edge_key(T, c, lo, hi); return hi; });
	sort_by(val, n, [&](int32_t c) { int32_t lo, hi; edge_key(T, c, lo, hi); return lo; });
	for (int64_t s = 0; s < n; s++) {
		const int r = group_entry(T, n, val, s, C->opposite);
		C->counts[0] += r & 1;
		C->counts[1] += (r >> 1) & 1;
	}
	for (int64_t c = 0; c < n; c++) val[c] = (int32_t)c;
	sort_by(val, n, [&](int32_t c) { return corner_node(T, c); });
	for (int64_t s = 0; s < n; s++) {
		C->ringTris[s] = val[s] / 3;
		csr_offsets(C->triOff, T.nNodes, s, n, s ? corner_node(T, val[s - 1]) : -1, corner_node(T, val[s]), (int32_t)s, (int32_t)n);
	}
	for (int64_t p = 0; p < m; p++) val[p] = (int32_t)p;
	sort_by(val, m, [&](int32_t p) { return pair_neighbour(T, p); });
	sort_by(val, m, [&](int32_t p) { return pair_node(T, p); });
	int32_t* rank = exact<int32_t>(m);
	int32_t total = 0;
	for (int64_t s = 0; s < m; s++) {
		rank[s] = total;
		total += pair_is_first(T, val, s);
	}
	C->ringLen = total;
	C->ringNodes = exact<int32_t>(total);
	for (int64_t s = 0; s < m; s++) {
		const int32_t first = pair_is_first(T, val, s), r = rank[s];
		if (first) C->ringNodes[r] = pair_neighbour(T, val[s]);
		csr_offsets(C->nodeOff, T.nNodes, s, m, s ? pair_node(T, val[s - 1]) : -1, pair_node(T, val[s]), r, r + first);
	}
	free(val);
	free(rank);
	return true;
}

static void release(Conn* C) {
	free(C->opposite); free(C->nodeOff); free(C->ringNodes); free(C->triOff); free(C->ringTris);
}

int main(int argc, char** argv) {
	if (argc < 4) return 2;
	const std::string mode = argv[1];
	FILE* in = fopen(argv[2], "rb");
	FILE* out = fopen(argv[3], "wb");
	if (!in || !out) return 2;
	int64_t nt[2];
	if (fread(nt, 8, 2, in) != 2) return 2;
	const int64_t n = nt[0], t = nt[1];
	float *pos = exact<float>(3 * n), *normal = exact<float>(3 * n);
	int32_t *flags = exact<int32_t>(n), *tri = exact<int32_t>(3 * t), *tflags = exact<int32_t>(t);
	if (fread(pos, 4, 3 * n, in) != (size_t)(3 * n) || fread(normal, 4, 3 * n, in) != (size_t)(3 * n) || fread(flags, 4, n, in) != (size_t)n ||
	    fread(tri, 4, 3 * t, in) != (size_t)(3 * t) || fread(tflags, 4, t, in) != (size_t)t)
		return 2;
	const Tris T = {t, t, n, tri};
	Conn C;
	const bool ok = build(T, &C);
	if (mode == "conn") {
		fwrite(C.counts, 4, 4, out);
		if (ok) {
			const int32_t len = (int32_t)C.ringLen;
			fwrite(C.opposite, 4, 3 * t, out); fwrite(C.nodeOff, 4, n + 1, out); fwrite(&len, 4, 1, out); fwrite(C.ringNodes, 4, len, out);
			fwrite(C.triOff, 4, n + 1, out); fwrite(C.ringTris, 4, 3 * t, out);
		}
	} else if (!ok || C.counts[0]) {
		return 3;
	} else if (mode == "smooth") {
		if (argc < 7) return 2;
		const float str = (float)atof(argv[4]), minLength = (float)atof(argv[5]);
		float* temp = exact<float>(3 * n);
		for (int step = 0; step < atoi(argv[6]); step++) {
			const Nodes N = {n, n, pos, flags};
			for (int64_t p = 0; p < n; p++) {
				float o[3];
				smooth_node(N, C.nodeOff, C.ringNodes, C.triOff, p, str, minLength, o);
				for (int c = 0; c < 3; c++) temp[c * n + p] = o[c];
			}
			for (int64_t p = 0; p < n; p++)
				if (!(flags[p] & 1))
					for (int c = 0; c < 3; c++) pos[c * n + p] = temp[c * n + p];
		}
		double* terms = exact<double>(4 * t);
		for (int64_t q = 0; q < t; q++) {
			double v[4];
			volume_terms(T, n, pos, q, v);
			for (int c = 0; c < 4; c++) terms[c * t + q] = v[c];
		}
		fwrite(pos, 4, 3 * n, out);
		fwrite(terms, 8, 4 * t, out);
		free(temp); free(terms);
	} else if (mode == "kill") {
		if (argc < 5 || C.counts[1]) return 3;
		const int elements = atoi(argv[4]);
		int32_t *label = exact<int32_t>(t), *size = exact<int32_t>(t), *taint = exact<int32_t>(t), *below = exact<int32_t>(t);
		for (int64_t q = 0; q < t; q++) label[q] = (int32_t)q;
		for (bool changed = true; changed;) {          // sweeps of "take the smallest label across an edge" to the fixed point
			changed = false;
			for (int64_t q = 0; q < t; q++)
				for (int c = 0; c < 3; c++) {
					const int32_t op = C.opposite[3 * q + c];
					if (op >= 0 && label[op / 3] < label[q]) {
						label[q] = label[op / 3];
						changed = true;
					}
				}
		}
		for (int64_t q = 0; q < t; q++) size[label[q]]++;
		int32_t K = 0;
		for (int64_t q = 0; q < t; q++) {
			below[q] = K;
			taint[q] = size[label[q]] < elements ? 1 : 0;
			K += taint[q];
		}
		int32_t *first = exact<int32_t>(n), *crank = exact<int32_t>(3 * t), *deleted = exact<int32_t>(n);
		for (int64_t v = 0; v < n; v++) first[v] = INT_MAX;
		for (int64_t c = 3 * t - 1; c >= 0; c--)
			if (taint[c / 3]) first[corner_node(T, c)] = (int32_t)c;
		int32_t D = 0;
		for (int64_t c = 0; c < 3 * t; c++) {
			crank[c] = D;
			D += is_first_tainted_corner(T, taint, first, c);
		}
		for (int64_t c = 0; c < 3 * t; c++)
			if (is_first_tainted_corner(T, taint, first, c)) deleted[crank[c]] = corner_node(T, c);
		const int64_t newT = t - K, newsize = n - D;
		for (int64_t h = 0; h < newT; h++)
			if (taint[h]) {
				const int64_t q = hole_source(taint, below, t, K, h);
				for (int c = 0; c < 3; c++) tri[c * t + h] = tri[c * t + q];
				tflags[h] = tflags[q];
			}
		int32_t *spotFlag = exact<int32_t>(D), *keptFlag = exact<int32_t>(D), *spotRank = exact<int32_t>(D), *keptRank = exact<int32_t>(D);
		int32_t *spot = exact<int32_t>(D), *newIndex = exact<int32_t>(D);
		int32_t a = 0, b = 0;
		for (int64_t i = 0; i < D; i++) {
			spotFlag[i] = deleted[i] < newsize ? 1 : 0;
			keptFlag[i] = first[newsize + i] == INT_MAX ? 1 : 0;
			spotRank[i] = a;
			keptRank[i] = b;
			a += spotFlag[i];
			b += keptFlag[i];
		}
		for (int64_t i = 0; i < D; i++)
			if (spotFlag[i]) spot[spotRank[i]] = deleted[i];
		for (int64_t i = 0; i < D; i++) {
			const int32_t j = newIndex[i] = node_new_index(keptFlag, keptRank, spot, i);
			if (j < 0) continue;
			for (int c = 0; c < 3; c++) {
				pos[c * n + j] = pos[c * n + newsize + i];
				normal[c * n + j] = normal[c * n + newsize + i];
			}
			flags[j] = flags[newsize + i];
		}
		for (int c = 0; c < 3; c++)
			for (int64_t q = 0; q < newT; q++) {
				const int64_t v = tri[c * t + q];
				if (v >= newsize) tri[c * t + q] = newIndex[v - newsize];
			}
		const int64_t counts[2] = {newsize, newT};
		fwrite(counts, 8, 2, out);
		for (int c = 0; c < 3; c++) fwrite(pos + c * n, 4, newsize, out);
		for (int c = 0; c < 3; c++) fwrite(normal + c * n, 4, newsize, out);
		fwrite(flags, 4, newsize, out);
		for (int c = 0; c < 3; c++) fwrite(tri + c * t, 4, newT, out);
		fwrite(tflags, 4, newT, out);
		free(label); free(size); free(taint); free(below); free(first); free(crank); free(deleted);
		free(spotFlag); free(keptFlag); free(spotRank); free(keptRank); free(spot); free(newIndex);
	} else {
		return 2;
	}
	release(&C);
	fclose(in); fclose(out);
	free(pos); free(normal); free(flags); free(tri); free(tflags);
	return 0;
}
