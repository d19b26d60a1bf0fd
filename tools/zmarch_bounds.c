/*
 * tools/zmarch_bounds.c -- the oracle's semi-Lagrange / MacCormack entry points on the thin grids of cases.ZMARCH_DIMS
 * (tests/cases.py), under AddressSanitizer and UBSan, as a stand-alone CPU program.  tests/test_gpu_base_edges.py::test_zmarch_depths
 * compares the HIP kernels with the oracle at these shapes; this program shows first that the oracle itself stays inside its arrays
 * there (every grid is an exact-size heap block, so one cell too far is reported).
 *
 *   gcc -O1 -g -std=gnu11 -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -Wno-unknown-pragmas -o /tmp/zmarch_bounds tools/zmarch_bounds.c -lm && /tmp/zmarch_bounds
 *
 * Exit status 0 and one "ok" line per shape = clean.  Other shapes: give them as arguments, `zmarch_bounds 7x6x3 ...`.
 * The destination grids start as NaN: a cell that a step leaves unwritten is reported too (the package hands these steps
 * temp grids that were not cleared).
 */
#include "../oracle/manta_oracle.c"

/* the shapes of cases.ZMARCH_DIMS -- tests/test_base_edges_inputs.py keeps the two lists equal */
static const int SHAPES[][3] = {{5, 4, 3}, {5, 4, 5}, {9, 7, 4}, {9, 7, 8}, {33, 5, 6}, {6, 5, 2}};

static uint32_t g_rng = 12345u;
static float urand(void) { /* [-1, 1) */
	g_rng = g_rng * 1664525u + 1013904223u;
	return (float)(g_rng >> 8) * (2.f / 16777216.f) - 1.f;
}
static float* grid(int64_t n, int fill_nan) {
	float* g = (float*)malloc(sizeof(float) * (size_t)n);
	for (int64_t q = 0; q < n; q++) g[q] = fill_nan ? NAN : urand();
	return g;
}
static int64_t count_nan(const float* g, int64_t n) {
	int64_t c = 0;
	for (int64_t q = 0; q < n; q++) c += isnan(g[q]) ? 1 : 0;
	return c;
}

static int run_shape(int sx, int sy, int sz) {
	const int64_t n = (int64_t)sx * sy * sz;
	int bad = 0;
	int32_t* flags = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
	for (int k = 0; k < sz; k++)
		for (int j = 0; j < sy; j++)
			for (int i = 0; i < sx; i++) {
				const int wall = i == 0 || j == 0 || k == 0 || i == sx - 1 || j == sy - 1 || k == sz - 1;
				flags[((int64_t)k * sy + j) * sx + i] = wall ? MF_OBSTACLE : (urand() < -0.6f ? MF_EMPTY : MF_FLUID);
			}
	float* vel = grid(3 * n, 0);
	for (int64_t q = 0; q < 3 * n; q++) vel[q] *= 2.5f; /* up to 2.5 cells per step: traces leave the grid on every side */
	for (int ncomp = 1; ncomp <= 3; ncomp += 2) {
		for (int orderTrace = 1; orderTrace <= 2; orderTrace++) {
			float *src = grid(ncomp * n, 0), *fwd = grid(ncomp * n, 1), *bwd = grid(ncomp * n, 1), *dst = grid(ncomp * n, 1);
			int rc;
			if (ncomp == 1) {
				rc = mf_semi_lagrange_real(sx, sy, sz, vel, fwd, src, 0.9f, orderTrace, 1, NULL);
				rc |= mf_semi_lagrange_real(sx, sy, sz, vel, bwd, fwd, -0.9f, orderTrace, 1, NULL);
			} else {
				rc = mf_semi_lagrange_vec3(sx, sy, sz, vel, fwd, src, 0.9f, orderTrace, 1, NULL);
				rc |= mf_semi_lagrange_vec3(sx, sy, sz, vel, bwd, fwd, -0.9f, orderTrace, 1, NULL);
			}
			for (int clampMode = 1; clampMode <= 2; clampMode++)
				rc |= mf_maccormack_correct_clamp(sx, sy, sz, ncomp, flags, vel, dst, src, fwd, bwd, 0.8f, 0.9f, clampMode, NULL);
			const int64_t un = count_nan(fwd, ncomp * n) + count_nan(bwd, ncomp * n) + count_nan(dst, ncomp * n);
			if (rc || un) {
				printf("%dx%dx%d ncomp %d orderTrace %d: rc %d (%s), %lld cells left unwritten\n", sx, sy, sz, ncomp, orderTrace, rc,
				       rc ? mf_last_error() : "", (long long)un);
				bad = 1;
			}
			free(src);
			free(fwd);
			free(bwd);
			free(dst);
		}
	}
	free(vel);
	free(flags);
	if (!bad) printf("%dx%dx%d ok\n", sx, sy, sz);
	return bad;
}

int main(int argc, char** argv) {
	int bad = 0;
	if (argc > 1) {
		for (int a = 1; a < argc; a++) {
			int sx, sy, sz;
			if (sscanf(argv[a], "%dx%dx%d", &sx, &sy, &sz) != 3) {
				fprintf(stderr, "usage: %s [SXxSYxSZ ...]\n", argv[0]);
				return 2;
			}
			bad |= run_shape(sx, sy, sz);
		}
	} else {
		for (size_t q = 0; q < sizeof(SHAPES) / sizeof(SHAPES[0]); q++) bad |= run_shape(SHAPES[q][0], SHAPES[q][1], SHAPES[q][2]);
	}
	return bad;
}
