// mg_host.h -- what the two multigrid hierarchies (multigrid.hip: 3-D over mg3d_cells.h, mg2d.hip: 2-D over mg2d_cells.h) and their
// one driver (mg_driver.h) share below the level types: the vertex types, the small exact helpers of the per-vertex bodies
// (imin, imax, pow2inv, ordered_sum, set_rhs), the host side of the set-up (the bucket heap and the greedy coarse-vertex
// selection of genCoarseGrid) and the registry of live handles.  Nothing here launches anything: tools/mg2d_host_check.hip runs
// the same text on the host.
#pragma once
#include "common.h"
#include <algorithm>
#include <mutex>
#include <set>
#include <vector>

namespace mf {

enum : unsigned char { vtInactive = 0, vtActive = 1, vtActiveTrivial = 2, vtRemoved = 3, vtZero = 4, vtFree = 5 };   // multigrid.h:87-94

// the size of one level (sz == 1 on every level of a 2-D hierarchy)
struct MgDim {
	int sx, sy, sz, n;
};

#define MG_HD __host__ __device__ __forceinline__

constexpr int MAXL = 16;      // levels of a hierarchy at most

MG_HD int imin(int a, int b) { return a < b ? a : b; }
MG_HD int imax(int a, int b) { return a > b ? a : b; }
// 1 / (1 << k), k = 0..3: exact
MG_HD float pow2inv(int k) { return k == 0 ? 1.f : k == 1 ? 0.5f : k == 2 ? 0.25f : 0.125f; }

// knSetRhs (trivial rows scaled), multigrid.cpp:417-424, and knSet(x_0, 0), :458, at vertex v of level 0
template <class Lv>
MG_HD void set_rhs(const Lv& L, int v, const float* rhs) {
	float b = rhs[v];
	if (L.t[v] == vtActiveTrivial) b *= 1E-6f;
	L.b[v] = b;
	L.x[v] = 0.f;
}
// the sum of a[0..n) in index order, as the reference's serial loop forms it (the entries of inactive vertices are +0, which
// leaves a sum that started at +0 unchanged)
MG_HD double ordered_sum(const double* a, int n) {
	double s = 0.0;
	int i = 0;
	for (; i + 8 <= n; i += 8) {
		const double a0 = a[i], a1 = a[i + 1], a2 = a[i + 2], a3 = a[i + 3], a4 = a[i + 4], a5 = a[i + 5], a6 = a[i + 6], a7 = a[i + 7];
		s += a0; s += a1; s += a2; s += a3; s += a4; s += a5; s += a6; s += a7;
	}
	for (; i < n; i++) s += a[i];
	return s;
}

// The handles that a create entry gave out and its destroy entry has not taken back: a destroyed or foreign handle is refused
// without reading the memory it points to.
class LiveHandles {
	std::mutex mutex_;
	std::set<void*> live_;

  public:
	bool has(void* h) {
		std::lock_guard<std::mutex> lock(mutex_);
		return live_.count(h) != 0;
	}
	void insert(void* h) {
		std::lock_guard<std::mutex> lock(mutex_);
		live_.insert(h);
	}
	void erase(void* h) {
		std::lock_guard<std::mutex> lock(mutex_);
		live_.erase(h);
	}
};

// The bucket min-heap of genCoarseGrid (NKMinHeap, multigrid.cpp:57-186): one doubly linked list per key; set_key puts an ID at
// the HEAD of its new key's list and pop_min takes the head of the smallest non-empty key -- among equal keys the vertex whose
// key was set last comes out first.  The selection depends on that order.
struct BucketHeap {
	int N, K, size, minKey;
	std::vector<int> key, prev, next;      // entries 0..K-1: list heads; K + id: the IDs
	BucketHeap(int n, int k) : N(n), K(k), size(0), minKey(-1), key(n + k, -1), prev(n + k, -1), next(n + k, -1) {}
	int get_key(int id) const { return key[K + id]; }
	void advance_min() {
		for (; minKey < K; minKey++)
			if (next[minKey] != -1) break;
	}
	void unlink(int e) {
		const int pr = prev[e], su = next[e];
		next[pr] = su;
		if (su != -1) prev[su] = pr;
	}
	void set_key(int id, int k) {
		const int e = K + id;
		if (key[e] == k) return;
		if (key[e] != -1) {
			unlink(e);
			if (key[e] == minKey) {
				if (size == 1) minKey = -1;
				else advance_min();
			}
			size--;
		}
		key[e] = k;
		if (k == -1) {
			next[e] = prev[e] = -1;
			return;
		}
		size++;
		minKey = (minKey == -1) ? k : std::min(minKey, k);
		const int old = next[k];
		next[k] = e;
		prev[e] = k;
		next[e] = old;
		if (old != -1) prev[old] = e;
	}
	int pop_min() {
		const int e = next[minKey];
		unlink(e);
		key[e] = prev[e] = next[e] = -1;
		size--;
		if (size == 0) minKey = -1;
		else advance_min();
		return e - K;
	}
};

// genCoarseGrid + knActivateCoarseVertices, multigrid.cpp:507-578, on host copies of the type bytes; returns the active count.
// On a 2-D hierarchy (sz == 1 on both levels) the z loops run once and the keys stay within 1..4.  The reference sizes the
// heap with 5 keys there (:531) and with 9 in 3-D; the key array only has to hold the largest key, and the lists of the keys
// that never occur stay empty, so the pop order is the same with 9 for both.
inline int select_coarse(const MgDim& F, const unsigned char* tf, const MgDim& C, unsigned char* tc) {
	std::fill(tc, tc + C.n, (unsigned char)vtFree);
	BucketHeap heap(F.n, 9);
	for (int v = 0; v < F.n; v++) {
		if (tf[v] == vtInactive) continue;
		const int X = v % F.sx, Y = (v / F.sx) % F.sy, Z = v / (F.sx * F.sy);
		heap.set_key(v, 1 << ((X & 1) + (Y & 1) + (Z & 1)));
	}
	while (heap.size > 0) {
		const int v = heap.pop_min();
		const int X = v % F.sx, Y = (v / F.sx) % F.sy, Z = v / (F.sx * F.sy);
		bool vdone = false;
		for (int iz = Z / 2; iz <= (Z + 1) / 2; iz++)
		for (int iy = Y / 2; iy <= (Y + 1) / 2; iy++)
		for (int ix = X / 2; ix <= (X + 1) / 2; ix++) {
			const int i = ix + C.sx * (iy + C.sy * iz);
			if (tc[i] != vtFree) continue;
			if (vdone) tc[i] = vtRemoved;
			else {
				tc[i] = vtZero;
				vdone = true;
			}
			const int r0x = std::max(0, ix * 2 - 1), r0y = std::max(0, iy * 2 - 1), r0z = std::max(0, iz * 2 - 1);
			const int r1x = std::min(F.sx - 1, ix * 2 + 1), r1y = std::min(F.sy - 1, iy * 2 + 1), r1z = std::min(F.sz - 1, iz * 2 + 1);
			for (int rz = r0z; rz <= r1z; rz++)
			for (int ry = r0y; ry <= r1y; ry++)
			for (int rx = r0x; rx <= r1x; rx++) {
				const int r = rx + F.sx * (ry + F.sy * rz);
				const int k = heap.get_key(r);
				if (k > 1) heap.set_key(r, k - 1);
				else if (k > -1) heap.set_key(r, -1);
			}
		}
	}
	int active = 0;
	for (int i = 0; i < C.n; i++) {
		tc[i] = (tc[i] == vtZero) ? vtActive : vtInactive;      // free -> removed -> inactive
		active += tc[i] == vtActive;
	}
	return active;
}

}  // namespace mf
