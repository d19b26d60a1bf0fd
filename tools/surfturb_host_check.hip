// tools/surfturb_host_check.hip -- the per-point bodies of mantaflow_amd/csrc/surfturb_cells.h run on the HOST: every launch of
// surfturb.hip replaced by a serial loop, the cell sort by a serial counting sort, the scans by serial sums, as a stand-alone program
// for the host sanitizers.  tools/surfturb_host_check.py drives it with the recorded stages and calls of tests/golden/surfturb.npz and
// compares with the reference's states.  It makes no HIP call and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -fsanitize=address,undefined tools/surfturb_host_check.hip -o <scratch>/surfturb_host_check
//   python tools/surfturb_host_check.py <scratch>/surfturb_host_check
//
// usage: surfturb_host_check <call|params|STAGE> <in.bin> <out.bin>      STAGE: adddelete accel normals regularize constrain waves advect
//   in:  int64 h[8] = res, frameCount, nb, Rc, Rs (0: derive them), nc, n, mDeletes, mDeleteChunk is h[8]: nine int64 in all;
//        float args[13] (outerRadius, surfaceDensity, nb, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude,
//        waveMaxFrequency, waveMaxSeedingAmplitude, centre, radius, step); int32 grid[res^3]; coarse pos[3][nc], flag[nc], prev[3][nc];
//        surface pos[3][n], flag[n], normals[3][n], real[5][n] (H, DtH, source, seed, seedAmp)
//   out: int64 o[6] = n, mDeletes, mDeleteChunk, displaced, iterations, directions; the surface arrays as above; displaced[3][o[3]];
//        int64 stats[iterations][6] (added, rounds, kills of the three passes, compressed); params: float par[32], int32 R[2], dirs
// Every array is a heap block of its exact size, so an index outside it is an AddressSanitizer report.
#include "../mantaflow_amd/csrc/surfturb_cells.h"
#include <stdlib.h>
#include <string>
#include <vector>

using namespace mf;
using namespace mf::surfturb;

namespace mf {      // common.h declares them; this program has no runtime.hip
thread_local char g_err[512];
int fail(const char*, ...) { return 1; }
}

typedef std::vector<float> VF;
typedef std::vector<int32_t> VI;

static void relayout(VF& a, int ncomp, int64_t oldn, int64_t newn) {
	VF b((size_t)(ncomp * newn), 0.f);
	for (int c = 0; c < ncomp; c++)
		for (int64_t i = 0; i < (oldn < newn ? oldn : newn); i++) b[c * newn + i] = a[c * oldn + i];
	a.swap(b);
}
static V3 get3(const VF& a, int64_t n, int64_t i) { return {a[i], a[n + i], a[2 * n + i]}; }
static void put3(VF& a, int64_t n, int64_t i, V3 v) { a[i] = v.x; a[n + i] = v.y; a[2 * n + i] = v.z; }

struct List {
	int R = 1;
	VI start, ids;
	Cells view() const { return {R, start.data(), ids.data()}; }
	void build(const Par& par, int64_t n, const VF& pos, int64_t stride) {       // a serial stable counting sort
		const int64_t nc = (int64_t)R * R * R;
		start.assign((size_t)nc + 1, 0);
		ids.assign((size_t)(n ? n : 1), 0);
		std::vector<int64_t> cell((size_t)n);
		for (int64_t i = 0; i < n; i++) {
			cell[i] = cell_of(V3{pos[i], pos[stride + i], pos[2 * stride + i]}, par.res, R);
			start[cell[i] + 1]++;
		}
		for (int64_t c = 0; c < nc; c++) start[c + 1] += start[c];
		VI fill(start.begin(), start.end() - 1);
		for (int64_t i = 0; i < n; i++) ids[fill[cell[i]]++] = (int32_t)i;
	}
};

struct Sim {
	Par par;
	int res = 0, nb = 0;
	int64_t nc = 0, n = 0, deletes = 0, chunk = 0;
	VI grid, cflag, flag;
	VF cpos, prev, pos, normals, real, displaced;
	List LC, LS;
	std::vector<int64_t> stats;
	Pts coarse() const { return {nc, nc, cpos.data(), cflag.data()}; }
	Pts surf() const { return {n, n, pos.data(), flag.data()}; }
	void resize(int64_t m) {
		relayout(pos, 3, n, m);
		relayout(normals, 3, n, m);
		relayout(real, 5, n, m);
		flag.resize((size_t)m, 0);
		n = m;
	}
	void coarse_list(bool of_prev) { LC.build(par, nc, of_prev ? prev : cpos, nc); }
	void surface_list(bool empty = false) { LS.build(par, empty ? 0 : n, pos, n); }

	void init_fines() {
		const int64_t nd = direction_table(par, 0, nullptr);
		VF dirs((size_t)(3 * nd));
		direction_table(par, nd, dirs.data());
		VF out;
		for (int64_t p = 0; p < nc; p++)
			for (int64_t d = 0; d < nd; d++) {
				V3 o;
				if (init_fine(par, LC.view(), coarse(), res, res, res, grid.data(), p, V3{dirs[3 * d], dirs[3 * d + 1], dirs[3 * d + 2]}, o)) {
					out.push_back(o.x); out.push_back(o.y); out.push_back(o.z);
				}
			}
		const int64_t m = (int64_t)out.size() / 3;
		n = 0;
		pos.clear(); normals.clear(); real.clear(); flag.clear();
		resize(m);
		for (int64_t i = 0; i < m; i++) put3(pos, n, i, V3{out[3 * i], out[3 * i + 1], out[3 * i + 2]});
		deletes = 0;
		chunk = m / 20;
	}
	void advect() {
		const Pts pv = {nc, nc, prev.data(), nullptr};
		VF np_(pos);
		for (int64_t i = 0; i < n; i++)
			if (active(surf(), i)) put3(np_, n, i, advect_point(par, LC.view(), pv, coarse(), get3(pos, n, i)));
		pos.swap(np_);
	}
	void add_delete() {
		int64_t st[6] = {0, 0, 0, 0, 0, 0};
		const int64_t n0 = n;
		VF cand;
		for (int64_t i = 0; i < n0; i++) {
			V3 o;
			if (add_candidate(par, LC.view(), coarse(), LS.view(), surf(), i, o)) { cand.push_back(o.x); cand.push_back(o.y); cand.push_back(o.z); }
		}
		if (deletes > chunk) abort();       // the first doCompress never compresses
		for (int64_t i = 0; i < n0; i++) flag[i] &= ~PNEW;
		const int64_t k = (int64_t)cand.size() / 3;
		resize(n0 + k);
		for (int64_t i = 0; i < k; i++) {
			put3(pos, n, n0 + i, V3{cand[3 * i], cand[3 * i + 1], cand[3 * i + 2]});
			flag[n0 + i] = PNEW;
		}
		st[0] = k;
		// delete pass 1 in rounds, reading the state of the round before
		VI a((size_t)(n ? n : 1), 0), b(a);
		bool undecided = n > 0;
		while (undecided) {
			undecided = false;
			for (int64_t i = 0; i < n; i++) {
				int32_t s = a[i];
				if (s == 0) {
					s = greedy_decide(par, LS.view(), surf(), a.data(), i);
					if (s == 0) undecided = true;
				}
				b[i] = s;
			}
			a.swap(b);
			st[1]++;
		}
		VI nf(flag);
		for (int64_t i = 0; i < n; i++) {
			const int r = delete_coarse(par, LC.view(), coarse(), get3(pos, n, i));
			const int k1 = a[i] == 2;
			st[2] += k1; st[3] += r & 1; st[4] += (r >> 1) & 1;
			if (k1 || r) nf[i] |= PDELETE;
		}
		flag.swap(nf);
		deletes += st[2] + st[3] + st[4];
		if (deletes > chunk) {      // ParticleSystem::compress: the tail fills the holes
			st[5] = 1;
			int64_t next = n;
			for (int64_t i = 0; i < n; i++)
				while (flag[i] & PDELETE) {
					next--;
					put3(pos, n, i, get3(pos, n, next));
					put3(normals, n, i, get3(normals, n, next));
					for (int c = 0; c < 5; c++) real[c * n + i] = real[c * n + next];
					flag[i] = flag[next];
					flag[next] = 1 << 30;
				}
			resize(next);
			deletes = 0;
			chunk = n / 20;
		}
		for (int64_t i = 0; i < n; i++) flag[i] &= ~PNEW;
		stats.insert(stats.end(), st, st + 6);
	}
	void normals_stage() {
		for (int64_t i = 0; i < n; i++) put3(normals, n, i, surface_normal(par, LC.view(), coarse(), LS.view(), surf(), i));
		VF t((size_t)(3 * n));
		for (int64_t i = 0; i < n; i++) put3(t, n, i, averaged_normal(par, LS.view(), surf(), normals.data(), i));
		normals.swap(t);
	}
	void regularize() {
		VF dens((size_t)(n ? n : 1)), t((size_t)(3 * n));
		for (int64_t i = 0; i < n; i++) dens[i] = surface_density(par, LS.view(), surf(), i);
		for (int64_t i = 0; i < n; i++) put3(t, n, i, surface_displacement(par, LS.view(), surf(), normals.data(), dens.data(), i));
		for (int64_t i = 0; i < 3 * n; i++) pos[i] = pos[i] + t[i];
	}
	void constrain() {
		for (int64_t i = 0; i < n; i++) put3(pos, n, i, constrained(par, LC.view(), coarse(), get3(pos, n, i)));
	}
	void waves() {
		float *H = real.data(), *D = H + n, *src = H + 2 * n, *seed = H + 3 * n, *amp = H + 4 * n;
		VF tv((size_t)(3 * n)), tf((size_t)(n ? n : 1));
		for (int64_t i = 0; i < n; i++) H[i] += seed[i];
		for (int64_t i = 0; i < n; i++) put3(tv, n, i, wave_normal(par, LS.view(), surf(), normals.data(), H, i));
		for (int64_t i = 0; i < n; i++) tf[i] = wave_laplacian(par, LS.view(), surf(), normals.data(), H, tv.data(), i);
		for (int64_t i = 0; i < n; i++) evolve_wave(par, tf[i], seed[i], H[i], D[i]);
		for (int64_t i = 0; i < n; i++) tf[i] = surface_curvature(par, LS.view(), surf(), normals.data(), i);
		VF s2((size_t)(n ? n : 1));
		for (int64_t i = 0; i < n; i++) s2[i] = smooth_curvature(par, LS.view(), surf(), tf.data(), i);
		for (int64_t i = 0; i < n; i++) {
			src[i] = s2[i];
			seed_wave(par, src[i], seed[i], amp[i]);
		}
	}
	void iteration() {
		add_delete();
		surface_list();
		normals_stage();
		regularize();
		surface_list();
		constrain();
		surface_list();
	}
	void call(int frameCount) {
		if (frameCount == 0) {
			coarse_list(false);
			init_fines();
			surface_list(true);
			for (int it = 0; it < 6 * nb; it++) iteration();
			for (int c = 0; c < 5; c++)
				if (c != 2)
					for (int64_t i = 0; i < n; i++) real[c * n + i] = 0.f;
		} else {
			coarse_list(true);
			advect();
			surface_list();
			coarse_list(false);
			for (int it = 0; it < nb; it++) iteration();
			waves();
		}
		for (int64_t i = 0; i < nc; i++)
			if ((cflag[i] & (PNEW | PDELETE)) == 0) put3(prev, nc, i, get3(cpos, nc, i));
		std::vector<V3> d;
		for (int64_t i = 0; i < n; i++)
			if (active(surf(), i)) d.push_back(get3(pos, n, i) + get3(normals, n, i) * real[i]);
		displaced.assign(3 * d.size(), 0.f);
		for (size_t i = 0; i < d.size(); i++) put3(displaced, (int64_t)d.size(), (int64_t)i, d[i]);
	}
};

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t count) {
	v.resize(count);
	return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
	if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
	if (argc < 4) return 2;
	const std::string mode = argv[1];
	FILE* in = fopen(argv[2], "rb");
	if (!in) return 3;
	std::vector<int64_t> h;
	VF args;
	if (!rd(in, h, 9) || !rd(in, args, 13)) return 4;
	Sim S;
	S.res = (int)h[0];
	S.nb = (int)h[2];
	S.nc = h[5];
	S.n = h[6];
	S.deletes = h[7];
	S.chunk = h[8];
	const int frameCount = (int)h[1];
	S.par = derive_par(S.res, args[0], (int)args[1], args[3], args[4], args[5], args[6], args[7], args[8], args[9], args[10], args[11], args[12], frameCount);
	S.LC.R = h[3] ? (int)h[3] : cvt_x86(2.f * S.res / S.par.outerRadius);
	S.LS.R = h[4] ? (int)h[4] : cvt_x86(1.f * S.res / (2.f * S.par.meanFineDistance));
	const size_t cells = (size_t)S.res * S.res * S.res;
	if (!rd(in, S.grid, cells) || !rd(in, S.cpos, 3 * S.nc) || !rd(in, S.cflag, S.nc) || !rd(in, S.prev, 3 * S.nc) || !rd(in, S.pos, 3 * S.n) ||
	    !rd(in, S.flag, S.n) || !rd(in, S.normals, 3 * S.n) || !rd(in, S.real, 5 * S.n))
		return 4;
	fclose(in);
	FILE* out = fopen(argv[3], "wb");
	if (!out) return 3;
	int64_t nd = direction_table(S.par, 0, nullptr);
	if (mode == "params") {
		VF par(NPAR), dirs((size_t)(3 * nd));
		memcpy(par.data(), &S.par, sizeof(Par));
		direction_table(S.par, nd, dirs.data());
		const VI R = {S.LC.R, S.LS.R};
		wr(out, par);
		wr(out, R);
		wr(out, dirs);
		fclose(out);
		return 0;
	}
	if (mode == "call")
		S.call(frameCount);
	else {
		// a single stage sees the lists of the state it starts from: the coarse one over the positions (advect: over prev)
		S.coarse_list(mode == "advect");
		S.surface_list();
		if (mode == "adddelete") S.add_delete();
		else if (mode == "accel") {}
		else if (mode == "normals") S.normals_stage();
		else if (mode == "regularize") S.regularize();
		else if (mode == "constrain") S.constrain();
		else if (mode == "waves") S.waves();
		else if (mode == "advect") S.advect();
		else return 2;
	}
	const std::vector<int64_t> o = {S.n, S.deletes, S.chunk, (int64_t)S.displaced.size() / 3, (int64_t)S.stats.size() / 6, nd};
	wr(out, o);
	wr(out, S.pos);
	wr(out, S.flag);
	wr(out, S.normals);
	wr(out, S.real);
	wr(out, S.displaced);
	wr(out, S.stats);
	fclose(out);
	return 0;
}
