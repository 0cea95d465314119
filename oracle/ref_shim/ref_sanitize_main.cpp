// oracle/ref_shim/ref_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program round ref_driver.cpp for a host sanitizer pass
// (`make -C oracle ref-sanitize` builds it and the reference's files with
// -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all).
// It feeds the driver arrays read from raw little-endian files, so that the very
// inputs a test used can be replayed under the sanitizers, outside Python:
//
//   ref_sanitize expand PARENTS.f32 RNG.u32 OBSTACLES.f32 numDisc agentLength width height
//   ref_sanitize cells  XY.f32 R1Size N R2Size n
//   ref_sanitize goal   XY.f32 goalX goalY r
//   ref_sanitize cost   X0.f32 X1.f32
//   ref_sanitize motion BBMIN.f32 BBMAX.f32 OBSTACLES.f32
//
// Every command prints a checksum of what the driver returned and exits 0; a
// sanitizer report aborts it.  It confirms that the chosen inputs stay clear of the
// reference's undefined float -> int conversions and of reads past the arrays.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
void ref_expand(const float* parents, uint32_t* rng, int n, int numDisc, float agentLength, const float* obstacles,
                int count, float width, float height, float* children, uint8_t* valid);
void ref_cells(const float* xy, int n, float R1Size, int N, float R2Size, int nn, int* r1, int* r2);
void ref_goal(const float* xy, int n, const float* goal, float r, uint8_t* inside);
void ref_cost(const float* x0, const float* x1, int n, float* cost);
void ref_motion_valid(const float* bbMin, const float* bbMax, int n, const float* obstacles, int count,
                      uint8_t* valid);
}

template <typename T>
static std::vector<T> load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

static uint64_t sum(const void* p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

static int usage() {
    fprintf(stderr, "usage: ref_sanitize expand|cells|goal|cost|motion FILES... PARAMETERS...\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "expand" && argc == 9) {
        // exact-size arrays: a read or write past a row shows under the address sanitizer
        std::vector<float> par = load<float>(argv[2]), obs = load<float>(argv[4]);
        std::vector<uint32_t> rng = load<uint32_t>(argv[3]);
        const int n = (int)(par.size() / 7);
        if (rng.size() != (size_t)n * 6) return usage();
        std::vector<float> children((size_t)n * 7);
        std::vector<uint8_t> valid((size_t)n);
        ref_expand(par.data(), rng.data(), n, atoi(argv[5]), (float)atof(argv[6]), obs.data(), (int)(obs.size() / 4),
                   (float)atof(argv[7]), (float)atof(argv[8]), children.data(), valid.data());
        printf("expand %d rows, %d boxes: %016llx %016llx\n", n, (int)(obs.size() / 4),
               (unsigned long long)sum(children.data(), children.size() * 4),
               (unsigned long long)sum(valid.data(), valid.size()));
    } else if (cmd == "cells" && argc == 7) {
        std::vector<float> xy = load<float>(argv[2]);
        const int n = (int)(xy.size() / 2);
        std::vector<int> r1((size_t)n), r2((size_t)n);
        ref_cells(xy.data(), n, (float)atof(argv[3]), atoi(argv[4]), (float)atof(argv[5]), atoi(argv[6]), r1.data(),
                  r2.data());
        printf("cells %d rows: %016llx %016llx\n", n, (unsigned long long)sum(r1.data(), r1.size() * 4),
               (unsigned long long)sum(r2.data(), r2.size() * 4));
    } else if (cmd == "goal" && argc == 6) {
        std::vector<float> xy = load<float>(argv[2]);
        const int n = (int)(xy.size() / 2);
        const float goal[2] = {(float)atof(argv[3]), (float)atof(argv[4])};
        std::vector<uint8_t> inside((size_t)n);
        ref_goal(xy.data(), n, goal, (float)atof(argv[5]), inside.data());
        printf("goal %d rows: %016llx\n", n, (unsigned long long)sum(inside.data(), inside.size()));
    } else if (cmd == "cost" && argc == 4) {
        std::vector<float> x0 = load<float>(argv[2]), x1 = load<float>(argv[3]);
        const int n = (int)(x1.size() / 7);
        std::vector<float> cost((size_t)n);
        ref_cost(x0.data(), x1.data(), n, cost.data());
        printf("cost %d rows: %016llx\n", n, (unsigned long long)sum(cost.data(), cost.size() * 4));
    } else if (cmd == "motion" && argc == 5) {
        std::vector<float> lo = load<float>(argv[2]), hi = load<float>(argv[3]), obs = load<float>(argv[4]);
        const int n = (int)(lo.size() / 2);
        std::vector<uint8_t> valid((size_t)n);
        ref_motion_valid(lo.data(), hi.data(), n, obs.data(), (int)(obs.size() / 4), valid.data());
        printf("motion %d rows, %d boxes: %016llx\n", n, (int)(obs.size() / 4),
               (unsigned long long)sum(valid.data(), valid.size()));
    } else {
        return usage();
    }
    return 0;
}
