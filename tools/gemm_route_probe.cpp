// Prints the GEMM dispatcher's routing answers over a fixed grid of calls (tests/golden/gemm_routes.npz holds this program's output at a named commit
// as the byte array `text`; tests/test_gemm_route_host.py holds d4_gemm_route to it).  Host logic only: the pointers are fake, aligned and never
// dereferenced, nothing is launched and no GPU is needed (the CU count falls back to 256, the MI355X's own).
//
//   hipcc -std=c++17 -Idreamer4_amd/csrc tools/gemm_route_probe.cpp -Ldreamer4_amd -ld4hip -Wl,-rpath,$PWD/dreamer4_amd -o gemm_route_probe
//   ./gemm_route_probe <commit> | python -c "import sys, numpy as np; np.savez_compressed(sys.argv[1], text=np.frombuffer(sys.stdin.buffer.read(), np.uint8))" gemm_routes.npz
//
// One line per (M, N, K, batch, rule_M, row map, forced code):   M N K batch rule_M map forced : <40 cells, no separator>
// The cells run over flags {0, 1, 2, 5, 8, 16, 24, 32} (outer) x weight kind {0 f32 only, 1 bf16 image, 2 bf16 image + Ab, 3 three planes, 4 two planes +
// scales} (inner).  A cell is four hex digits: two for the bits 1 gemm_rule_takes_v2, 2 gemm_rule_takes_x3sk, 4 gemm_h2_takes, 8 gemm_skinny_applicable,
// 16 gemm2_ksplit_rule, then two for the mask of gemm_config_valid(c, .), c = 0 .. 7.
// The call of a cell: A = 0x1000, W = 0x2000, C = 0x3000, lda = ldw = K, ldc = N, rms_eps = 1e-6; batch > 1: strideA = M K, strideW = N K, strideC = M N;
// kinds 1 - 4: Wb = 0x4000; kind 2: Ab = 0x5000; kinds 3, 4: wplane = N K batch; kind 4: wscale = 0x6000, strideWs = N; row map on: rm_Sc = 7, rm_lo = 3,
// rm_nr = 2.  The first block is every shape at batch 1, rule_M 0, no map, nothing forced; the second crosses the other axes over a thinned shape list in
// which every M, N and K of the grid still appears.
#include <stdio.h>
#include <stdint.h>
#include "kernels.h"

using namespace d4;

static const int kM[] = {1, 16, 17, 200, 256, 257, 512, 513, 1023, 1024, 3584, 8192};
static const int kN[] = {64, 192, 512, 1552, 2047, 2048, 2752, 5504};
static const int kK[] = {32, 72, 96, 128, 512, 1024, 2048};
static const int kFlags[] = {0, 1, 2, 5, 8, 16, 24, 32};
static const int kBatch[] = {1, 4};
static const int kRuleM[] = {0, 3584};
static const int kForced[] = {-1, 4, 106, 199, 302, 401};
enum { KINDS = 5 };

static GemmArgs make_call(int M, int N, int K, int flags, int kind, int batch, int rule_M, int map) {
    GemmArgs g{reinterpret_cast<const float*>(0x1000), K, reinterpret_cast<const float*>(0x2000), K, reinterpret_cast<float*>(0x3000), N,
               nullptr, nullptr, 0, M, N, K, flags, 1e-6f};
    g.batch = batch;
    if (batch > 1) { g.strideA = (int64_t)M * K; g.strideW = (int64_t)N * K; g.strideC = (int64_t)M * N; }
    if (kind >= 1) g.Wb = reinterpret_cast<const uint16_t*>(0x4000);
    if (kind == 2) g.Ab = reinterpret_cast<const uint16_t*>(0x5000);
    if (kind >= 3) g.wplane = (int64_t)N * K * batch;
    if (kind == 4) { g.wscale = reinterpret_cast<const float*>(0x6000); g.strideWs = N; }
    g.rule_M = rule_M;
    if (map) { g.rm_Sc = 7; g.rm_lo = 3; g.rm_nr = 2; }
    return g;
}

static void line(int M, int N, int K, int batch, int rule_M, int map, int forced) {
    printf("%d %d %d %d %d %d %d : ", M, N, K, batch, rule_M, map, forced);
    gemm_force_config(forced);
    for (int flags : kFlags)
        for (int kind = 0; kind < KINDS; ++kind) {
            const GemmArgs g = make_call(M, N, K, flags, kind, batch, rule_M, map);
            const int bits = (gemm_rule_takes_v2(g) ? 1 : 0) | (gemm_rule_takes_x3sk(g) ? 2 : 0) | (gemm_h2_takes(g) ? 4 : 0) |
                             (gemm_skinny_applicable(g) ? 8 : 0) | (gemm2_ksplit_rule(g) ? 16 : 0);
            int mask = 0;
            for (int c = 0; c < 8; ++c) mask |= gemm_config_valid(c, g) ? 1 << c : 0;
            printf("%02x%02x", bits, mask);
        }
    printf("\n");
    gemm_force_config(-1);
}

int main(int argc, char** argv) {
    printf("# GEMM dispatcher routes: tools/gemm_route_probe.cpp at commit %s\n", argc > 1 ? argv[1] : "(unnamed)");
    printf("# M N K batch rule_M map forced : cells over flags {0 1 2 5 8 16 24 32} x kind {0..4}; cell = bits(v2 1, x3sk 2, h2 4, skinny 8, ksplit 16) mask(config_valid 0..7)\n");
    for (int M : kM)
        for (int N : kN)
            for (int K : kK) line(M, N, K, 1, 0, 0, -1);
    for (int i = 0; i < 12; ++i)
        for (int j = 0; j < 2; ++j) {
            const int M = kM[i], N = kN[(3 * i + j) % 8], K = kK[(i + 2 * j) % 7];
            for (int batch : kBatch)
                for (int rule_M : kRuleM)
                    for (int map = 0; map < 2; ++map)
                        for (int forced : kForced)
                            if (batch != 1 || rule_M != 0 || map != 0 || forced != -1) line(M, N, K, batch, rule_M, map, forced);
        }
    return 0;
}
