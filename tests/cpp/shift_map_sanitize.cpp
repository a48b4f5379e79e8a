// AddressSanitizer / UBSan run of the host code behind rn_shift_warm_start / rn_get_shift_map (rapidnet_amd/csrc/shift_map.hpp, plain C++): the
// node correspondence of the shifted warm start on trees read from a file, written out for the caller to compare with the numpy restatement
// (tests/shift_oracle.py), plus the checks that need no second opinion: every entry is a node one stage below its node (the last stage onto
// itself), the children ranges tile the nodes, a caller's map is accepted exactly when its entries lie in [-1, nodes).  Arrays are allocated
// at their exact sizes, so an index one past an array is the sanitizer's to find.
// Input (argv[1]): the number of trees, then per tree `nodes N rootChild`, the parents (-1 for the root) and nodesPerStageCumul.
// Output: per tree one line with the map.  Built and run by tests/test_host_shift_map_sanitized.py; exit code 0 = clean.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rapidnet_amd/csrc/shift_map.hpp"

#define CHECK(c)                                                                                                        \
    do {                                                                                                                \
        if (!(c)) { std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); std::exit(2); }                \
    } while (0)

using namespace rn::shift;

int main(int argc, char **argv) {
    CHECK(argc == 2);
    std::FILE *in = std::fopen(argv[1], "r");
    CHECK(in != nullptr);
    int trees = 0, runs = 0;
    CHECK(std::fscanf(in, "%d", &trees) == 1);
    for (int t = 0; t < trees; t++) {
        int nodes = 0, N = 0, rootChild = 0;
        CHECK(std::fscanf(in, "%d %d %d", &nodes, &N, &rootChild) == 3 && nodes >= 1 && N >= 1);
        std::vector<int> parent((size_t)nodes), cum((size_t)N + 1), stage((size_t)nodes), map((size_t)nodes, -7);
        for (int i = 0; i < nodes; i++) CHECK(std::fscanf(in, "%d", &parent[i]) == 1);
        for (int k = 0; k <= N; k++) CHECK(std::fscanf(in, "%d", &cum[k]) == 1);
        CHECK(cum[0] == 0 && cum[N] == nodes);
        std::vector<int> start, count;
        child_ranges(parent.data(), nodes, start, count);
        int next = 1;
        for (int i = 0; i < nodes; i++) if (count[i]) { CHECK(start[i] == next); next += count[i]; }      // the ranges tile nodes 1 .. nodes - 1
        CHECK(next == nodes && root_children(parent.data(), nodes) == count[0]);
        stages_of(cum.data(), N, stage.data());
        CHECK(rootChild >= 0 && rootChild < (count[0] > 0 ? count[0] : 1));
        build_map(parent.data(), nodes, rootChild, map.data());
        CHECK(map_ok(map.data(), (size_t)nodes));
        for (int i = 0; i < nodes; i++) {
            CHECK(map[i] >= 0 && map[i] < nodes);
            CHECK(stage[map[i]] == (stage[i] + 1 < N ? stage[i] + 1 : N - 1));
            if (i > 0 && count[map[parent[i]]] > 0) CHECK(parent[map[i]] == map[parent[i]]);      // a child of what the parent inherits from
        }
        {   // a caller's map: -1 is allowed, anything else outside the tree is not
            std::vector<int> own(map);
            own[(size_t)nodes - 1] = -1;
            CHECK(map_ok(own.data(), (size_t)nodes));
            own[(size_t)nodes - 1] = nodes;
            CHECK(!map_ok(own.data(), (size_t)nodes));
            own[(size_t)nodes - 1] = -2;
            CHECK(!map_ok(own.data(), (size_t)nodes));
        }
        for (int i = 0; i < nodes; i++) std::printf(i ? " %d" : "%d", map[i]);
        std::printf("\n");
        runs++;
    }
    std::fclose(in);
    {   // the most probable child: the first of equal maxima
        const double p[5] = {0.1, 0.3, 0.3, 0.2, 0.1}, q[1] = {1.0}, r[3] = {0.2, 0.2, 0.6};
        CHECK(most_probable(p, 5) == 1 && most_probable(q, 1) == 0 && most_probable(r, 3) == 2 && most_probable(p, 1) == 0);
    }
    std::printf("shift map runs %d\n", runs);
    return 0;
}
