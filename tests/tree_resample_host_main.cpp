// The host twin of the resample (include/sbmp/tree_resample.h) as a stand-alone program, for a
// sanitizer build (tests/test_tree_resample.py compiles it with -fsanitize=address,undefined and
// runs it once).  Crafted chains in exact-size heap arrays: path lengths 1, 2, 3, 64, 65 and 257,
// power-of-two durations with every grid time on a step or an edge boundary, a period longer
// than the path, and durations that are no time (0, -1, NaN, +inf, the smallest denormal).  Every
// output array has exactly the size the sizing call returned, so a sample written one place too
// far, or a T_k read past the path, lands where AddressSanitizer stops the program.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sbmp/tree_resample.h"

namespace {
constexpr int kDisc = 10;

int fail(const char* what, long long a, long long b) {
    std::printf("FAILED: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

struct Chain {
    int rows;
    float* state;
    float* ctrl;
    int* parent;
    // row r the child of row r - 1 under (a, steering, durations[r - 1]); a duration that is no
    // time leaves the row on its parent's state
    Chain(int n, const float* durations, int numDisc) : rows(n) {
        state = new float[4 * (size_t)n];
        ctrl = new float[4 * (size_t)n];
        parent = new int[(size_t)n];
        state[0] = 1.0f, state[1] = 5.0f, state[2] = 0.3f, state[3] = 1.0f;
        ctrl[0] = ctrl[1] = ctrl[2] = ctrl[3] = 0.0f;
        parent[0] = -1;
        std::vector<float> steps(4 * (size_t)numDisc);
        for (int r = 1; r < n; ++r) {
            float* c = ctrl + 4 * (size_t)r;
            c[0] = (r & 1) ? 1.0f : -1.0f;
            c[1] = 0.05f;
            c[2] = durations[r - 1];
            c[3] = 0.0f;
            parent[r] = r - 1;
            const bool time = c[2] > 0.0f && std::isfinite(c[2]);
            if (time) sbmp::traceCarControls(state + 4 * (size_t)(r - 1), numDisc, 1.0f, c[0], c[1], c[2], steps.data());
            for (int q = 0; q < 4; ++q)
                state[4 * (size_t)r + q] = time ? steps[4 * (size_t)(numDisc - 1) + q] : state[4 * (size_t)(r - 1) + q];
        }
    }
    ~Chain() {
        delete[] state;
        delete[] ctrl;
        delete[] parent;
    }
};

// Sizes, allocates exactly, fills; checks what every path must satisfy.  Returns the sample count
// of the first request through *first, 0 for success.
int run(const Chain& c, int agent, int numDisc, const int* nodes, int count, double period, int depthBound,
        std::vector<int>* countsOut, std::vector<int>* edgesOut, std::vector<double>* timesOut,
        std::vector<float>* statesOut) {
    int* counts = new int[(size_t)count];
    uint8_t* status = new uint8_t[(size_t)count];
    const long long total = sbmp::resample_paths_host(c.state, c.ctrl, c.parent, depthBound, agent, numDisc, 1.0f, nodes,
                                                      count, period, counts, status, false, nullptr, nullptr, nullptr);
    if (total < 0) return fail("the sizing call refused", total, 0);
    float* states = new float[4 * (size_t)total];
    int* edges = new int[(size_t)total];
    double* times = new double[(size_t)total];
    if (sbmp::resample_paths_host(c.state, c.ctrl, c.parent, depthBound, agent, numDisc, 1.0f, nodes, count, period,
                                  nullptr, nullptr, true, states, edges, times) != total)
        return fail("the filling call's total differs", total, 0);
    long long at = 0;
    for (int i = 0; i < count; ++i) {
        if (status[i] != SBMP_PATH_OK) {
            if (counts[i] != 0) return fail("a request without a path has samples", i, counts[i]);
            continue;
        }
        if (counts[i] < 2) return fail("an OK path has fewer than two samples", i, counts[i]);
        if (times[at] != 0.0) return fail("a path does not start at time 0", i, 0);
        for (int m = 1; m < counts[i]; ++m)
            if (!(times[at + m] >= times[at + m - 1])) return fail("times descend", i, m);
        const long long last = at + counts[i] - 1;
        if (edges[last] != nodes[i]) return fail("the end sample's edge is not the node", i, edges[last]);
        for (int q = 0; q < 4; ++q)
            if (sbmp::f2u(states[4 * last + q]) != sbmp::f2u(c.state[4 * (size_t)nodes[i] + q]))
                return fail("the end sample is not the node as stored", i, q);
        for (int m = 0; m < counts[i]; ++m)
            if (edges[at + m] < 0 || edges[at + m] > nodes[i]) return fail("an edge off the path", i, edges[at + m]);
        at += counts[i];
    }
    if (at != total) return fail("the counts do not sum to the total", at, total);
    if (countsOut) countsOut->assign(counts, counts + count);
    if (edgesOut) edgesOut->assign(edges, edges + total);
    if (timesOut) timesOut->assign(times, times + total);
    if (statesOut) statesOut->assign(states, states + 4 * total);
    delete[] counts;
    delete[] status;
    delete[] states;
    delete[] edges;
    delete[] times;
    return 0;
}
}  // namespace

int main() {
    // path lengths 1, 2, 3, 64, 65, 257 of one chain, two periods, both agents
    {
        std::vector<float> d(256, 0.07f);
        Chain c(257, d.data(), kDisc);
        const int nodes[8] = {0, 1, 2, 63, 64, 256, -1, 64};
        for (double period : {0.05, 0.013, 100.0}) {
            std::vector<int> counts;
            if (run(c, SBMP_AGENT_CAR, kDisc, nodes, 8, period, c.rows, &counts, nullptr, nullptr, nullptr)) return 1;
            if (counts[0] != 2 || counts[6] != 0 || counts[4] != counts[7]) return fail("counts", counts[0], counts[6]);
            if (period == 100.0)
                for (int i = 0; i < 6; ++i)
                    if (counts[i] != 2) return fail("a period longer than the path", i, counts[i]);
            if (run(c, SBMP_AGENT_POINT, kDisc, nodes, 8, period, c.rows, nullptr, nullptr, nullptr, nullptr)) return 1;
        }
        // depthBound one short of the chain: no samples
        const int last[1] = {256};
        std::vector<int> counts;
        if (run(c, SBMP_AGENT_CAR, kDisc, last, 1, 0.05, 256, &counts, nullptr, nullptr, nullptr)) return 1;
        if (counts[0] != 0) return fail("a deep path has samples", counts[0], 0);
    }
    // durations 1.0 with numDisc 8: dt = 0.125 exactly
    {
        std::vector<float> d(6, 1.0f);
        Chain c(7, d.data(), 8);
        const int last[1] = {6};
        std::vector<int> counts, edges;
        std::vector<double> times;
        std::vector<float> states;
        if (run(c, SBMP_AGENT_CAR, 8, last, 1, 0.125, 0 + c.rows, &counts, &edges, &times, nullptr)) return 1;
        if (counts[0] != 50) return fail("step boundaries: samples", counts[0], 50);
        for (int m = 0; m < 48; ++m)
            if (edges[(size_t)m] != m / 8 + 1 || times[(size_t)m] != m * 0.125) return fail("step boundaries", m, edges[(size_t)m]);
        if (run(c, SBMP_AGENT_CAR, 8, last, 1, 1.0, c.rows, &counts, &edges, &times, &states)) return 1;
        if (counts[0] != 8) return fail("edge boundaries: samples", counts[0], 8);
        for (int m = 0; m < 6; ++m) {
            if (edges[(size_t)m] != m + 1) return fail("edge boundaries", m, edges[(size_t)m]);
            for (int q = 0; q < 4; ++q)
                if (states[4 * (size_t)m + q] != c.state[4 * (size_t)m + q]) return fail("edge boundaries: not the stored row", m, q);
        }
    }
    // durations that are no time
    {
        const float inf = std::numeric_limits<float>::infinity();
        const float d[9] = {std::numeric_limits<float>::denorm_min(), 0.3f, 0.0f, 0.2f, -1.0f, std::nanf(""), 0.25f, inf, 0.4f};
        Chain c(10, d, kDisc);
        const int last[1] = {9};
        for (double period : {0.05, 0.013, 0.3, 1e-3}) {
            std::vector<int> counts, edges;
            std::vector<double> times;
            if (run(c, SBMP_AGENT_CAR, kDisc, last, 1, period, c.rows, &counts, &edges, &times, nullptr)) return 1;
            double T = 0.0;
            for (float e : {d[0], d[1], d[3], d[6], d[8]}) T += (double)e;
            if (times.back() != T) return fail("bad durations add time", 0, 0);
            if (counts[0] != (int)std::floor(T / period) + 2) return fail("bad durations: samples", counts[0], 0);
            for (int e : edges)
                if (e == 3 || e == 5 || e == 6 || e == 8) return fail("a bad edge was selected", e, 0);
            if (edges[0] != 1 || edges[1] == 1) return fail("the denormal edge holds t = 0 alone", edges[0], edges[1]);
        }
    }
    std::printf("ok\n");
    return 0;
}
