// shift_map.hpp -- the node correspondence of the shifted warm start (rn_shift_warm_start, rn_get_shift_map; shift_warm_start.inc): which node's
// multiplier every node of the scenario tree inherits when the horizon recedes by one stage along one child of the root.  Host-only code,
// purely topological (no probabilities), tested without a GPU (tests/cpp/shift_map_sanitize.cpp, against a numpy restatement of the rule).
//
// The tree as the contexts hold it: nodes numbered stage by stage, parent[i] < i the 0-based parent (-1 for the root, node 0), the children
// of a node contiguous and in the order of their parents.
#pragma once
#include <cstddef>
#include <vector>

namespace rn {
namespace shift {

// first child and number of children of every node
inline void child_ranges(const int *parent, int nodes, std::vector<int> &start, std::vector<int> &count) {
    start.assign((size_t)nodes, 0); count.assign((size_t)nodes, 0);
    for (int i = 1; i < nodes; i++) {
        const int par = parent[i];
        if (count[par] == 0) start[par] = i;
        count[par]++;
    }
}
inline int root_children(const int *parent, int nodes) {
    int n = 0;
    for (int i = 1; i < nodes; i++) n += parent[i] == 0;
    return n;
}
// m(root) = child number rootChild of the root (the root itself when it is a leaf); for the r-th child j of i: child number min(r, nc - 1)
// of m(i) when m(i) has nc > 0 children, else m(i) -- the last stage repeats.  rootChild must lie in [0, root_children) (0 for a lone root).
inline void build_map(const int *parent, int nodes, int rootChild, int *map) {
    std::vector<int> start, count;
    child_ranges(parent, nodes, start, count);
    map[0] = count[0] > 0 ? start[0] + rootChild : 0;
    for (int i = 0; i < nodes; i++) {      // parents come before their children
        const int mi = map[i], nc = count[mi];
        for (int r = 0; r < count[i]; r++) map[start[i] + r] = nc > 0 ? start[mi] + (r < nc - 1 ? r : nc - 1) : mi;
    }
}
// a caller's map: every entry a node of the tree, or -1 for "start this node from zero"
inline bool map_ok(const int *map, size_t nodes) {
    for (size_t i = 0; i < nodes; i++) if (map[i] < -1 || (long long)map[i] >= (long long)nodes) return false;
    return true;
}
// the child of the root with the largest probability, ties to the lowest index; p = the probabilities of the root's nc children in child order
inline int most_probable(const double *p, int nc) {
    int best = 0;
    for (int r = 1; r < nc; r++) if (p[r] > p[best]) best = r;
    return best;
}
// stage of every node from nodesPerStageCumul [N + 1]
inline void stages_of(const int *cum, int N, int *stage) {
    for (int k = 0; k < N; k++) for (int i = cum[k]; i < cum[k + 1]; i++) stage[i] = k;
}

}  // namespace shift
}  // namespace rn
