// reinit_cells.h -- the per-cell and per-entry bodies of reinit.hip as __host__ __device__ functions, and the literal serial march as host
// code: the kernels call the bodies with one thread per cell or per list entry, mf_reinit_march_serial and a stand-alone host program
// (tools/reinit_host_check.hip) call the same text in serial loops, where the host sanitizers can watch every index.  Contract and
// fp32 / fp64 map: DESIGN.md section 18.  Built with -ffp-contract=off.  Reference: levelset.cpp:32-85, 122-228, fastmarch.cpp:23-221,
// fastmarch.h.
#pragma once
#include "common.h"
#include <vector>

#ifndef MF_HD
#define MF_HD __host__ __device__ __forceinline__
#endif

namespace mf {
namespace reinit {

constexpr int FM_INITED = 1, FM_ONHEAP = 2;      // FastMarch::SpecialValues
constexpr int TYPE_EMPTY = 4;                    // FlagGrid::TypeEmpty
#ifndef MF_REINIT_DELTA
#define MF_REINIT_DELTA 0.125f
#endif
constexpr float DELTA = MF_REINIT_DELTA;         // width of a window of keys (speed only)

// one march: dir = -1 inward, +1 outward (TDIR); maxT = maxTime * dir; vel (SoA [3][n]) is null without transport; fm0 = the flags as
// InitFmIn / InitFmOut left them (the seeding reads them while it writes fm)
struct March {
	Dim d;
	float* phi;
	int32_t* fm;
	float* key;
	const int32_t* fm0;
	const int32_t* flags;
	float* vel;
	float maxT;
	int dir, ignoreWalls, obsType;
	int32_t* epoch;      // the window in which a cell popped (0: not popped by the march in rounds); null in the serial march
};

// COMP::compare: x lies beyond y in the march's direction
MF_HD bool beyond(int dir, float x, float y) { return dir > 0 ? x > y : x < y; }
// the heap's order, fastmarch.h:99-124: a pops before b.  Time first, then (z, y, x), mirrored for the inward march
MF_HD bool precedes(int dir, float ta, int64_t a, float tb, int64_t b) {
	if (fabsf(ta - tb) > 0.f) return dir > 0 ? ta < tb : ta > tb;
	return dir > 0 ? a < b : a > b;
}
MF_HD bool in_window(int dir, float t, float te) { return dir > 0 ? t < te : t > te; }
MF_HD float window_end(int dir, float t) { return dir > 0 ? t + DELTA : t - DELTA; }
MF_HD bool is_wall(const March& m, int64_t idx) { return m.ignoreWalls && (m.flags[idx] & m.obsType) != 0; }
MF_HD bool interior(const Dim& d, int i, int j, int k) {
	return i >= 1 && i < d.sx - 1 && j >= 1 && j < d.sy - 1 && (d.is3d ? (k >= 1 && k < d.sz - 1) : k == 0);
}
MF_HD void cell_ijk(const Dim& d, int64_t idx, int& i, int& j, int& k) {
	const unsigned t = (unsigned)idx / (unsigned)d.sx;
	i = (int)((unsigned)idx - t * (unsigned)d.sx);
	j = (int)(t % (unsigned)d.sy);
	k = (int)(t / (unsigned)d.sy);
}
// float sqrt, correctly rounded on host and device alike (a double sqrt rounded once more is the correctly rounded float sqrt)
MF_HD float sqrt_f32(float x) { return (float)sqrt((double)x); }

// calculateDistance, fastmarch.cpp:34-130, for a cell whose six neighbours exist.  inited(q) says whether q counts as FlagInited.
// w[6] = mWeights (+x, -x, +y, -y, +z, -z)
template <class In>
MF_HD float calc_distance(const Dim& d, const float* phi, int dir, const In& inited, int64_t idx, float w[6]) {
	const int64_t st[3] = {1, d.Y, d.Z};
	int invcnt = 0, okcnt = 0;
	float v[3] = {0.f, 0.f, 0.f}, ax[3] = {0.f, 0.f, 0.f};
	for (int c = 0; c < 3; c++) {
		w[2 * c] = w[2 * c + 1] = 0.f;
		if (c == 2 && !d.is3d) {
			invcnt++;
			continue;
		}
		if (inited(idx + st[c])) {           // the + neighbour wins over the - neighbour
			ax[c] = phi[idx + st[c]];
			v[okcnt++] = ax[c];
			w[2 * c] = 1.f;
		} else if (inited(idx - st[c])) {
			ax[c] = phi[idx - st[c]];
			v[okcnt++] = ax[c];
			w[2 * c + 1] = 1.f;
		} else
			invcnt++;
	}
	float ret = -1000.f;                     // InvalidTime(): three invalid axes, which no touched cell has
	const float fdir = (float)dir;
	if (invcnt == 0) {
		const float ca = v[0], cb = v[1], cc = v[2];
		const float e = ca * ca + cb * cb - cb * cc + cc * cc - ca * (cb + cc);
		const double q = -2. * (double)e + 3;
		const float cs = (float)(0. < q ? q : 0.);
		const float sum = ca + cb + cc + fdir * sqrt_f32(cs);
		ret = (float)(0.333333 * (double)sum);
	} else if (invcnt == 1) {
		const double q = 2. - (double)((v[1] - v[0]) * (v[1] - v[0]));
		const float cs = (float)(0. < q ? q : 0.);
		const float sum = v[0] + v[1] + fdir * sqrt_f32(cs);
		ret = (float)(0.5 * (double)sum);
	} else if (invcnt == 2) {
		return v[0] + fdir;                  // the one weight stays 1
	} else
		return ret;
	for (int c = 0; c < 3; c++) {
		const float f = fabsf(ret - ax[c]);
		w[2 * c] *= f;
		w[2 * c + 1] *= f;
	}
	float norm = 0.f;
	for (int a = 0; a < 6; a++) norm += w[a];
	norm = (float)(1.0 / (double)norm);
	for (int a = 0; a < 6; a++) w[a] *= norm;
	return ret;
}

// FmValueTransportVec3::transpTouch, fastmarch.h:74-83
MF_HD void transp_touch(const Dim& d, const int32_t* flags, float* vel, int64_t idx, const float w[6]) {
	if (!(flags[idx] & TYPE_EMPTY)) return;
	const int64_t off[6] = {1, -1, d.Y, -d.Y, d.Z, -d.Z};
	float val[3] = {0.f, 0.f, 0.f};
	for (int a = 0; a < (d.is3d ? 6 : 4); a++)
		if (w[a] > 0.f)
			for (int c = 0; c < 3; c++) val[c] = val[c] + vel[c * d.n + idx + off[a]] * w[a];
	if (flags[idx - 1] & TYPE_EMPTY) vel[idx] = val[0];
	if (flags[idx - d.Y] & TYPE_EMPTY) vel[d.n + idx] = val[1];
	if (d.is3d && (flags[idx - d.Z] & TYPE_EMPTY)) vel[2 * d.n + idx] = val[2];
}

struct InitedNow {
	const int32_t* fm;
	MF_HD bool operator()(int64_t q) const { return fm[q] == FM_INITED; }
};

// FastMarch::addToList(p, src) for an interior p, fastmarch.cpp:132-178; true when p goes on the heap (its key is then m.key[p])
MF_HD bool touch(const March& m, int64_t p, int64_t src) {
	if (m.fm[p] == FM_INITED) return false;
	if (beyond(m.dir, m.phi[src], m.maxT)) return false;
	float w[6];
	const InitedNow in = {m.fm};
	const float t = calc_distance(m.d, m.phi, m.dir, in, p, w);
	const bool found = m.fm[p] == FM_ONHEAP;
	if (found && beyond(m.dir, t, m.phi[p])) return false;     // an equal time overwrites
	m.fm[p] = FM_ONHEAP;
	m.phi[p] = t;
	if (m.vel) transp_touch(m.d, m.flags, m.vel, p, w);
	if (found) return false;
	m.key[p] = t;
	return true;
}

// one pop of performMarching, fastmarch.cpp:202-215: push(q) is told every neighbour that goes on the heap
template <class Push>
MF_HD void pop_cell(const March& m, int64_t c, const Push& push) {
	int i, j, k;
	cell_ijk(m.d, c, i, j, k);
	m.fm[c] = FM_INITED;
	const int di[6] = {-1, 1, 0, 0, 0, 0}, dj[6] = {0, 0, -1, 1, 0, 0}, dk[6] = {0, 0, 0, 0, -1, 1};
	for (int a = 0; a < (m.d.is3d ? 6 : 4); a++) {
		if (!interior(m.d, i + di[a], j + dj[a], k + dk[a])) continue;
		const int64_t q = c + di[a] + m.d.Y * dj[a] + m.d.Z * dk[a];
		if (touch(m, q, c)) push(q);
	}
}

// a window entry pops in this sub-round when no unpopped window entry within L1 distance 2 precedes it
MF_HD bool selectable(const March& m, int64_t c, float te) {
	int i, j, k;
	cell_ijk(m.d, c, i, j, k);
	const float t = m.key[c];
	const int rk = m.d.is3d ? 2 : 0;
	for (int dk = -rk; dk <= rk; dk++)
		for (int dj = -2; dj <= 2; dj++)
			for (int di = -2; di <= 2; di++) {
				const int l1 = (di < 0 ? -di : di) + (dj < 0 ? -dj : dj) + (dk < 0 ? -dk : dk);
				if (l1 == 0 || l1 > 2) continue;
				const int x = i + di, y = j + dj, z = k + dk;
				if (x < 0 || y < 0 || z < 0 || x >= m.d.sx || y >= m.d.sy || z >= m.d.sz) continue;
				const int64_t q = c + di + m.d.Y * dj + m.d.Z * dk;
				if (m.fm[q] != FM_ONHEAP) continue;
				const float tq = m.key[q];
				if (in_window(m.dir, tq, te) && precedes(m.dir, tq, q, t, c)) return false;
			}
	return true;
}

// the flag rule, asked of a cell as it goes on the heap in window w: a cell within L1 distance 2 that has popped in this window although
// its key comes after the new one.  (The cell that pushed it is one of those looked at.)
MF_HD bool late_conflict(const March& m, int64_t c, int w) {
	int i, j, k;
	cell_ijk(m.d, c, i, j, k);
	const float t = m.key[c];
	const int rk = m.d.is3d ? 2 : 0;
	for (int dk = -rk; dk <= rk; dk++)
		for (int dj = -2; dj <= 2; dj++)
			for (int di = -2; di <= 2; di++) {
				const int l1 = (di < 0 ? -di : di) + (dj < 0 ? -dj : dj) + (dk < 0 ? -dk : dk);
				if (l1 == 0 || l1 > 2) continue;
				const int x = i + di, y = j + dj, z = k + dk;
				if (x < 0 || y < 0 || z < 0 || x >= m.d.sx || y >= m.d.sy || z >= m.d.sz) continue;
				const int64_t q = c + di + m.d.Y * dj + m.d.Z * dk;
				if (m.epoch[q] == w && precedes(m.dir, t, c, m.key[q], q)) return true;
			}
	return false;
}

// ---- set-up passes, levelset.cpp:32-70 (all cells: a border cell of fm is 0, as in the reference's fresh grid) ----
MF_HD void init_fm(const March& m, int64_t idx, int i, int j, int k) {
	m.key[idx] = 0.f;
	if (m.epoch) m.epoch[idx] = 0;
	if (!interior(m.d, i, j, k)) {
		m.fm[idx] = 0;
		return;
	}
	const float v = m.phi[idx];
	const bool wall = is_wall(m, idx);
	if (m.dir < 0)
		m.fm[idx] = (v >= 0.f && !wall) ? FM_INITED : 0;
	else {
		m.fm[idx] = (v < 0.f && !wall) ? FM_INITED : 0;
		if (wall) m.phi[idx] = 0.f;
	}
}
MF_HD void set_uninitialized(const March& m, int64_t idx, int i, int j, int k, float val) {
	if (!interior(m.d, i, j, k)) return;
	if (m.fm[idx] != FM_INITED && !is_wall(m, idx)) m.phi[idx] = val;
}

// SetLevelsetBoundaries, fastmarch.cpp:181-193, per cell: what the serial i-fastest sweep leaves in cell (i, j, k), from the field as
// it was before the sweep.  The last test that applies wins; a source cell with a lower index has been swept already (so its own rule
// is followed), one with a higher index still holds its old value.
MF_HD float boundary_value(const Dim& d, const float* phi, int i, int j, int k) {
	for (;;) {
		if (d.is3d && k == d.sz - 1 && k > 0) {
			k--;
			continue;
		}
		if (d.is3d && k == 0) return phi[i + d.Y * j + d.Z * 1];
		if (j == d.sy - 1) {
			j--;
			continue;
		}
		if (j == 0) return phi[i + d.Y * 1 + d.Z * k];
		if (i == d.sx - 1) {
			i--;
			continue;
		}
		if (i == 0) return phi[1 + d.Y * j + d.Z * k];
		return phi[i + d.Y * j + d.Z * k];
	}
}

// ---- seeding, levelset.cpp:134-154, 168-215, order-free ----
// isAtInterface, levelset.cpp:72-85, on the flags as the Init pass left them: the cells the loop marks have the sign that does not count
MF_HD bool at_interface(const March& m, int i, int j, int k) {
	const int di[6] = {-1, 1, 0, 0, 0, 0}, dj[6] = {0, 0, -1, 1, 0, 0}, dk[6] = {0, 0, 0, 0, -1, 1};
	for (int a = 0; a < (m.d.is3d ? 6 : 4); a++) {
		const int x = i + di[a], y = j + dj[a], z = k + dk[a];
		if (x < 0 || y < 0 || z < 0 || x >= m.d.sx || y >= m.d.sy || z >= m.d.sz) continue;
		const int64_t q = x + m.d.Y * y + m.d.Z * z;
		if (m.fm0[q] != FM_INITED) continue;
		if (m.dir < 0 ? m.phi[q] >= 0.f : m.phi[q] < 0.f) return true;
	}
	return false;
}
// the loop marks this cell FlagInited (inward march, and outward without correctOuterLayer)
MF_HD bool is_marked(const March& m, int i, int j, int k) {
	if (!interior(m.d, i, j, k)) return false;
	const int64_t idx = i + m.d.Y * j + m.d.Z * k;
	if (m.fm0[idx] == FM_INITED || is_wall(m, idx)) return false;
	if (!at_interface(m, i, j, k)) return false;
	return !(m.dir > 0 && m.phi[idx] < 0.f);       // read last: only a cell at the interface keeps its value during the seeding
}

struct InitedSeed {
	int64_t q[6];
	bool in[6];
	MF_HD bool operator()(int64_t r) const {
		for (int a = 0; a < 6; a++)
			if (q[a] == r) return in[a];
		return false;
	}
};

// one cell of the interface seeding: marks it, or plays the touches it receives from its marked neighbours in the loop's order
// (k outer, j, i inner: ascending index), each with the inited set of its moment.  True when the cell goes on the heap.
MF_HD bool seed_interface(const March& m, int64_t idx, int i, int j, int k) {
	if (!interior(m.d, i, j, k)) return false;
	if (is_marked(m, i, j, k)) {
		m.fm[idx] = FM_INITED;
		return false;
	}
	if (is_wall(m, idx) || m.fm0[idx] == FM_INITED || at_interface(m, i, j, k)) return false;
	const int di[6] = {0, 0, -1, 1, 0, 0}, dj[6] = {0, -1, 0, 0, 1, 0}, dk[6] = {-1, 0, 0, 0, 0, 1};
	InitedSeed in;
	bool mk[6];
	for (int a = 0; a < 6; a++) {
		in.q[a] = -1;
		in.in[a] = mk[a] = false;
		if (!m.d.is3d && dk[a]) continue;
		in.q[a] = idx + di[a] + m.d.Y * dj[a] + m.d.Z * dk[a];
		mk[a] = is_marked(m, i + di[a], j + dj[a], k + dk[a]);
		in.in[a] = m.fm0[in.q[a]] == FM_INITED;
	}
	float cur = m.phi[idx], key = 0.f;
	bool onheap = false;
	for (int a = 0; a < 6; a++) {
		if (!mk[a]) continue;
		in.in[a] = true;
		if (!(m.dir < 0 ? cur < 0.f : cur > 0.f)) continue;
		if (beyond(m.dir, m.phi[in.q[a]], m.maxT)) continue;
		float w[6];
		const float t = calc_distance(m.d, m.phi, m.dir, in, idx, w);
		if (onheap && beyond(m.dir, t, cur)) continue;
		cur = t;
		if (m.vel) transp_touch(m.d, m.flags, m.vel, idx, w);
		if (!onheap) key = t;
		onheap = true;
	}
	if (!onheap) return false;
	m.phi[idx] = cur;
	m.fm[idx] = FM_ONHEAP;
	m.key[idx] = key;
	return true;
}

struct InitedStart {
	const int32_t* fm0;
	MF_HD bool operator()(int64_t q) const { return fm0[q] == FM_INITED; }
};

// one cell of the correctOuterLayer seeding, levelset.cpp:168-188: the inited set does not change, so every touch of a cell gives the
// same time and one stands for all
MF_HD bool seed_outer(const March& m, int64_t idx, int i, int j, int k) {
	if (!interior(m.d, i, j, k) || is_wall(m, idx) || m.fm0[idx] == FM_INITED) return false;
	const int64_t off[6] = {-1, 1, -m.d.Y, m.d.Y, -m.d.Z, m.d.Z};
	bool any = false;
	for (int a = 0; a < (m.d.is3d ? 6 : 4) && !any; a++) {
		const int64_t q = idx + off[a];
		if (m.fm0[q] != FM_INITED || is_wall(m, q)) continue;
		const float v = m.phi[q];
		any = v < 0.f && v >= -2.f && !beyond(m.dir, v, m.maxT);
	}
	if (!any) return false;
	float w[6];
	const InitedStart in = {m.fm0};
	const float t = calc_distance(m.d, m.phi, m.dir, in, idx, w);
	m.fm[idx] = FM_ONHEAP;
	m.phi[idx] = t;
	m.key[idx] = t;
	if (m.vel) transp_touch(m.d, m.flags, m.vel, idx, w);
	return true;
}

// ---- the literal serial march (host): doReinitMarch's seeding loops and performMarching with a binary heap of (key, cell) ----
struct SerialHeap {
	int dir;
	std::vector<float> t;
	std::vector<int64_t> c;
	bool before(size_t a, size_t b) const { return precedes(dir, t[a], c[a], t[b], c[b]); }
	void swap(size_t a, size_t b) {
		std::swap(t[a], t[b]);
		std::swap(c[a], c[b]);
	}
	void push(float time, int64_t cell) {
		t.push_back(time);
		c.push_back(cell);
		for (size_t a = t.size() - 1; a > 0 && before(a, (a - 1) / 2); a = (a - 1) / 2) swap(a, (a - 1) / 2);
	}
	int64_t pop() {
		const int64_t top = c[0];
		swap(0, t.size() - 1);
		t.pop_back();
		c.pop_back();
		for (size_t a = 0;;) {
			size_t b = a;
			if (2 * a + 1 < t.size() && before(2 * a + 1, b)) b = 2 * a + 1;
			if (2 * a + 2 < t.size() && before(2 * a + 2, b)) b = 2 * a + 2;
			if (b == a) break;
			swap(a, b);
			a = b;
		}
		return top;
	}
};

struct InitedLive {
	const int32_t* fm;
	bool operator()(int64_t q) const { return fm[q] == FM_INITED; }
};
static inline bool serial_at_interface(const March& m, int i, int j, int k) {
	March live = m;
	live.fm0 = m.fm;
	return at_interface(live, i, j, k);
}

// seeding, march and SetLevelsetBoundaries of one direction on host arrays, as the reference runs them; returns the number of pops.
// m.fm0 is not read.
static inline int64_t serial_march(const March& m, bool outer) {
	const Dim& d = m.d;
	SerialHeap heap;
	heap.dir = m.dir;
	const int di[6] = {-1, 1, 0, 0, 0, 0}, dj[6] = {0, 0, -1, 1, 0, 0}, dk[6] = {0, 0, 0, 0, -1, 1};
	const int nnb = d.is3d ? 6 : 4;
	auto add = [&](int i, int j, int k, int64_t src) {
		if (!interior(d, i, j, k)) return;
		const int64_t p = i + d.Y * j + d.Z * k;
		if (touch(m, p, src)) heap.push(m.key[p], p);
	};
	for (int k = d.is3d ? 1 : 0; k < (d.is3d ? d.sz - 1 : 1); k++)
		for (int j = 1; j < d.sy - 1; j++)
			for (int i = 1; i < d.sx - 1; i++) {
				const int64_t p = i + d.Y * j + d.Z * k;
				if (outer) {
					if (is_wall(m, p)) continue;
					for (int a = 0; a < nnb; a++) {
						const int64_t q = p + di[a] + d.Y * dj[a] + d.Z * dk[a];
						if (m.fm[q] != FM_INITED || is_wall(m, q)) continue;
						const float v = m.phi[q];
						if (v < 0 && v >= -2) add(i, j, k, q);
					}
					continue;
				}
				if (m.dir < 0 && m.fm[p] == FM_INITED) continue;
				if (is_wall(m, p)) continue;
				if (m.dir > 0 && m.phi[p] < 0) continue;
				if (!serial_at_interface(m, i, j, k)) continue;
				m.fm[p] = FM_INITED;
				for (int a = 0; a < nnb; a++) {
					const int x = i + di[a], y = j + dj[a], z = k + dk[a];
					const int64_t q = x + d.Y * y + d.Z * z;
					if (is_wall(m, q)) continue;
					if ((m.dir < 0 ? m.phi[q] < 0.f : m.phi[q] > 0.f) && !serial_at_interface(m, x, y, z)) add(x, y, z, p);
				}
			}
	int64_t pops = 0;
	while (!heap.t.empty()) {
		const int64_t c = heap.pop();
		pops++;
		pop_cell(m, c, [&](int64_t q) { heap.push(m.key[q], q); });
	}
	for (int k = 0; k < d.sz; k++)
		for (int j = 0; j < d.sy; j++)
			for (int i = 0; i < d.sx; i++) {
				float& v = m.phi[i + d.Y * j + d.Z * k];
				if (i == 0) v = m.phi[1 + d.Y * j + d.Z * k];
				if (i == d.sx - 1) v = m.phi[i - 1 + d.Y * j + d.Z * k];
				if (j == 0) v = m.phi[i + d.Y * 1 + d.Z * k];
				if (j == d.sy - 1) v = m.phi[i + d.Y * (j - 1) + d.Z * k];
				if (d.is3d) {
					if (k == 0) v = m.phi[i + d.Y * j + d.Z * 1];
					if (k == d.sz - 1) v = m.phi[i + d.Y * j + d.Z * (k - 1)];
				}
			}
	return pops;
}

// the whole call on host arrays through the serial marches (set-up passes included): what the reference computes.  fm / key / fm0 are
// scratch of n entries; pops[2] = (inward, outward)
static inline void serial_call(Dim d, float* phi, int32_t* fm, float* key, const int32_t* flags, float* vel, float maxTime, int ignoreWalls,
                               int outer, int obsType, int64_t pops[2]) {
	for (int dir = -1; dir <= 1; dir += 2) {
		const March m = {d, phi, fm, key, fm, flags, dir > 0 ? vel : nullptr, maxTime * (float)dir, dir, ignoreWalls, obsType, nullptr};
		for (int64_t idx = 0; idx < d.n; idx++) {
			int i, j, k;
			cell_ijk(d, idx, i, j, k);
			init_fm(m, idx, i, j, k);
		}
		pops[dir > 0] = serial_march(m, dir > 0 && outer);
		const float val = dir < 0 ? (float)(-(double)maxTime - 1.) : (float)((double)maxTime + 1.);
		for (int64_t idx = 0; idx < d.n; idx++) {
			int i, j, k;
			cell_ijk(d, idx, i, j, k);
			set_uninitialized(m, idx, i, j, k, val);
		}
	}
}

}  // namespace reinit
}  // namespace mf
