// The opening plan of a Halo2 proof, stated once for the prover (plonk_bn254.hip) and the verifier (plonk_verifier.cpp): which commitments are
// opened at which points, in create_proof's query order, and ProverSHPLONK's grouping of them (construct_intermediate_sets).  The two sides
// must agree on it byte for byte or proofs stop verifying.  Host only.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "host_fr.h"

namespace gl355 {

// one slot per opened commitment: [advice | permutation z | lookup z | lookup A' | lookup S' | fixed | sigma | h | random]
struct PlkSlots {
    uint32_t advice, perm_z, lookup_z, lookup_a, lookup_s, fixed, sigma, h, random, count;
    PlkSlots(uint32_t n_advice, uint32_t n_sets, uint32_t n_lookups, uint32_t n_fixed, uint32_t n_perm)
        : advice(0), perm_z(n_advice), lookup_z(perm_z + n_sets), lookup_a(lookup_z + n_lookups), lookup_s(lookup_a + n_lookups), fixed(lookup_s + n_lookups),
          sigma(fixed + n_fixed), h(sigma + n_perm), random(h + 1), count(random + 1) {}
};

// x omega^r on the domain of 2^k rows
struct PlkRotate {
    Fr omega, omega_inv;
    explicit PlkRotate(uint32_t k) : omega(Fr::root_of_unity(k)), omega_inv(omega.inv()) {}
    Fr operator()(Fr x, int32_t r) const {                  // |r| is at most the blinding factors + 1: products, not a 256-bit power
        for (int64_t i = r < 0 ? -(int64_t)r : r; i > 0; i--) x = x * (r < 0 ? omega_inv : omega);
        return x;
    }
};

// slot opened at point = x omega^rot; `query`: for an advice / fixed column, the index of the column query that asks for it
struct PlkOpening { uint32_t slot; int32_t rot; uint32_t query; Fr point; };

using PlkQueries = std::vector<std::pair<int32_t, int32_t>>;              // (column, rotation)

// the opening queries in create_proof's order (`bf`: blinding factors, the last usable row is at rotation -(bf + 1))
inline std::vector<PlkOpening> plk_opening_queries(const PlkSlots& sl, const PlkQueries& advice_q, const PlkQueries& fixed_q, uint32_t bf, const PlkRotate& rotate, const Fr& x) {
    std::vector<PlkOpening> o;
    auto open = [&](uint32_t slot, int32_t rot, uint32_t query = 0) { o.push_back({slot, rot, query, rotate(x, rot)}); };
    const uint32_t n_sets = sl.lookup_z - sl.perm_z, n_lookups = sl.lookup_a - sl.lookup_z;
    const int32_t last = -(int32_t)(bf + 1);
    for (uint32_t q = 0; q < advice_q.size(); q++) open(sl.advice + advice_q[q].first, advice_q[q].second, q);
    for (uint32_t s = 0; s < n_sets; s++) { open(sl.perm_z + s, 0); open(sl.perm_z + s, 1); }
    for (uint32_t s = n_sets; s-- > 0;) if (s + 1 < n_sets) open(sl.perm_z + s, last);
    for (uint32_t l = 0; l < n_lookups; l++) {
        open(sl.lookup_z + l, 0); open(sl.lookup_a + l, 0); open(sl.lookup_s + l, 0);
        open(sl.lookup_a + l, -1); open(sl.lookup_z + l, 1);
    }
    for (uint32_t q = 0; q < fixed_q.size(); q++) open(sl.fixed + fixed_q[q].first, fixed_q[q].second, q);
    for (uint32_t j = sl.sigma; j < sl.h; j++) open(j, 0);
    open(sl.h, 0); open(sl.random, 0);
    return o;
}

// construct_intermediate_sets over a query sequence: the commitments in first-appearance order, each with its sorted distinct points (the
// order halo2curves' Ord gives Fr); the rotation sets = the distinct point sets in first-appearance order, with their members; all points
struct PlkRotationSets {
    struct Com { uint32_t slot; std::vector<Fr> pts; std::vector<size_t> first; };      // first[i]: the first query that opens pts[i]
    struct Set { std::vector<Fr> pts; std::vector<size_t> coms; };                      // members: indices into `coms`
    std::vector<Com> coms;
    std::vector<Set> sets;
    std::vector<Fr> all_points;                                                         // sorted
    std::vector<size_t> same;                                                           // per query: the first query of the same (slot, point)
    PlkRotationSets(const std::vector<PlkOpening>& queries, uint32_t n_slots) : same(queries.size()) {
        auto sort_with = [](std::vector<Fr>& p, std::vector<size_t>* tag) {
            for (size_t i = 1; i < p.size(); i++)
                for (size_t j = i; j > 0 && p[j].less_than(p[j - 1]); j--) { std::swap(p[j], p[j - 1]); if (tag) std::swap((*tag)[j], (*tag)[j - 1]); }
        };
        std::vector<int> com_of(n_slots, -1);
        for (size_t q = 0; q < queries.size(); q++) {
            const PlkOpening& o = queries[q];
            if (com_of[o.slot] < 0) { com_of[o.slot] = (int)coms.size(); coms.push_back({o.slot, {}, {}}); }
            Com& c = coms[com_of[o.slot]];
            const size_t i = std::find(c.pts.begin(), c.pts.end(), o.point) - c.pts.begin();
            if (i == c.pts.size()) { c.pts.push_back(o.point); c.first.push_back(q); }
            same[q] = c.first[i];
        }
        for (size_t ci = 0; ci < coms.size(); ci++) {
            Com& c = coms[ci];
            sort_with(c.pts, &c.first);
            size_t s = 0;
            while (s < sets.size() && sets[s].pts != c.pts) s++;
            if (s == sets.size()) sets.push_back({c.pts, {}});
            sets[s].coms.push_back(ci);
            for (auto& p : c.pts) if (!has(all_points, p)) all_points.push_back(p);
        }
        sort_with(all_points, nullptr);
    }
    static bool has(const std::vector<Fr>& v, const Fr& p) { return std::find(v.begin(), v.end(), p) != v.end(); }
};

}  // namespace gl355
