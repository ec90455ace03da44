// SURVEY 8(f) N4, the verifying half: halo2_proofs' verify_proof::<KZGCommitmentScheme<Bn256>, VerifierSHPLONK<_>, _, Keccak256Transcript,
// SingleStrategy<_>> as chip/native_chip/test_utils.rs:82-93 runs it on every proof create_proof_checked makes (verifier_api.rs:77-92), over
// the descriptor blob gl355_plonk_keygen takes.  Order of work, after the published verifier (plonk/verifier.rs, the argument verifiers,
// poly/kzg/multiopen/shplonk/verifier.rs):
//   transcript    vk digest and instances in; advice, lookup, permutation, vanishing and quotient commitments read, theta beta gamma y x squeezed
//                 in the prover's order; every point 64 big-endian bytes (canonical, on the curve), every scalar 32 bytes below r
//   evaluations   read; instance columns evaluated from the public values (Lagrange form)
//   expressions   the quotient's evaluation at x: the gate program interpreted once over the evaluations, permutation and lookup terms, all folded with y
//   SHPLONK       y v h1 u h2; commitments grouped into rotation sets as the prover groups them; L + u h2 as ONE list of (scalar, point) terms
//                 -- the quotient's pieces, the key's commitments and [1] G1 included -- so the group work is a single MSM
//   pairing       e(L + u h2, G2) e(-h2, [s] G2) = 1 (host_bn254_pairing.cpp).  Nothing here takes the SRS secret.
// A batch keeps the terms of its proofs apart, weighs proof b with a 128-bit rho_b and sums everything in one MSM -- on the device
// (gl355_bn254_g1_msm, bn254_msm.hip) from PLONK_VERIFY_DEVICE_MSM_MIN terms on -- and one two-pair pairing check.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gl355.h"
#include "blinding.cuh"
#include "host_fr.h"
#include "host_pairing.h"
#include "plonk_desc.h"
#include "plonk_openings.h"

using namespace gl355;

namespace {

thread_local std::string g_error;
thread_local double g_stage_ms[3] = {0, 0, 0};          // transcript + expressions, MSM, pairing of the thread's last verify call

// The term count from which an MSM of the batch verifier goes to the device when a context is given.  Below it the host sum is used.
// Measured on an MI355X host (`python tools/halo2_bench.py --batch`, msm_sweep; profiles/halo2_native_verify.txt), both MSMs of a batch,
// gl355_bn254_g1_msm from host arrays against bn254_g1_msm_host, terms: device / host ms
//     83: 0.61 / 1.40    140: 0.92 / 2.16    254: 1.26 / 3.52    482: 1.64 / 5.77    938: 1.01 / 9.99    1850: 1.66 / 17.7    7322: 3.45 / 64.5
// The device call won at every count measured, so the constant is the smallest of them (one proof of the reference's chip shape: 57 proof
// points + 26 of the key); nothing below 83 terms was measured, and those sums stay on the host.  Either side gives the same point, so the
// constant changes time only.  GL355_PLONK_VERIFY_DEVICE_MSM_MIN in the environment replaces it (include/gl355.h).
constexpr uint64_t PLONK_VERIFY_DEVICE_MSM_MIN = 83;

constexpr uint32_t STREAM_BATCH_WEIGHTS = 0x21, STREAM_PARAMS_POWERS = 0x22, STREAM_PARAMS_LAGRANGE = 0x23;

typedef std::array<uint64_t, 8> G1Words;

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct gl355_plonk_vk : PlkDesc {                                         // the parsed descriptor (plonk_desc.h), and what the verifier adds
    std::vector<uint32_t> perm_query;                                     // plk_perm_queries: the query (of its kind) that reads the column at rotation 0
    std::vector<uint64_t> key_points;                                     // fixed | sigma commitments | [1] G1, affine
    uint64_t s_g2[16];
};

void gl355::plonk_verify_set_error(const std::string& why) { g_error = why; }

namespace {

int32_t bad_arg(const char* why) { g_error = why; return GL355_E_INVALID_ARG; }

// ---- the transcript's reading side -------------------------------------------------------------------------------------------------------
struct Reader {
    const uint8_t* p;
    uint64_t len, pos = 0;
    KeccakTranscript tr;
    const char* err = nullptr;
    bool point(G1Words& out) {
        if (len - pos < 64) { err = "proof too short (point)"; return false; }
        KeccakTranscript::from_be32(p + pos, out.data()); KeccakTranscript::from_be32(p + pos + 32, out.data() + 4);
        if (!bn254_g1_valid_host(out.data())) { err = "a point of the proof is not canonical or not on the curve"; return false; }
        tr.buf.insert(tr.buf.end(), p + pos, p + pos + 64);
        pos += 64;
        return true;
    }
    bool scalar(Fr& out) {
        if (len - pos < 32) { err = "proof too short (scalar)"; return false; }
        uint64_t w[4];
        KeccakTranscript::from_be32(p + pos, w);
        if (Fr::geq_m(w)) { err = "a scalar of the proof is not below r"; return false; }
        out = Fr::from_words(w);
        tr.buf.insert(tr.buf.end(), p + pos, p + pos + 32);
        pos += 32;
        return true;
    }
};

void batch_invert(std::vector<Fr>& v) {                 // Montgomery's trick; a zero stays zero
    std::vector<Fr> pre(v.size());
    Fr acc = Fr::one();
    for (size_t i = 0; i < v.size(); i++) { pre[i] = acc; if (!v[i].is_zero()) acc = acc * v[i]; }
    acc = acc.inv();
    for (size_t i = v.size(); i-- > 0;) {
        if (v[i].is_zero()) continue;
        const Fr t = acc * pre[i];
        acc = acc * v[i];
        v[i] = t;
    }
}

// What one proof leaves for the group work: L + u h2 = sum_i proof_scalars[i] proof_points[i] + sum_j key_scalars[j] key_points[j], and h2
struct Prepared {
    std::vector<G1Words> points;
    std::vector<Fr> scalars;
    std::vector<Fr> key_scalars;
    G1Words h2;
};

// everything of verify_proof up to the pairing.  false: rejected, *why says at which step
bool prepare(const gl355_plonk_vk* vk, const uint64_t* instances, const uint32_t* lens, const uint8_t* proof, uint64_t proof_len, Prepared& out, const char** why) {
    const uint64_t n = vk->n, u_rows = vk->usable;
    const PlkRotate rotate(vk->k);
    const Fr &omega = rotate.omega, &omega_inv = rotate.omega_inv;
    Reader rd{proof, proof_len};
    auto fail = [&](const char* w) { *why = w; return false; };
    rd.tr.common_scalar(vk->digest);
    std::vector<std::vector<Fr>> inst(vk->n_instance);
    {
        uint64_t off = 0;
        for (uint32_t c = 0; c < vk->n_instance; c++) {
            if (lens[c] > u_rows) return fail("more instance values than usable rows");
            for (uint32_t i = 0; i < lens[c]; i++) { inst[c].push_back(Fr::from_words(instances + 4 * (off + i))); rd.tr.common_scalar(inst[c].back()); }
            off += lens[c];
        }
    }
    std::vector<G1Words>& pts = out.points;
    pts.clear();
    auto read_point = [&]() -> int { G1Words w; if (!rd.point(w)) return -1; pts.push_back(w); return (int)pts.size() - 1; };
#define RP(var) const int var = read_point(); if (var < 0) return fail(rd.err)
#define RS(var) if (!rd.scalar(var)) return fail(rd.err)
    std::vector<int> advice_c(vk->n_advice);
    for (auto& c : advice_c) { RP(t); c = t; }
    const Fr theta = rd.tr.squeeze_challenge();
    std::vector<std::array<int, 3>> lookups_c(vk->n_lookups);             // permuted input, permuted table, product
    for (auto& lc : lookups_c) { RP(a); RP(s); lc[0] = a; lc[1] = s; }
    const Fr beta = rd.tr.squeeze_challenge();
    const Fr gamma = rd.tr.squeeze_challenge();
    std::vector<int> perm_c(vk->n_sets);
    for (auto& c : perm_c) { RP(t); c = t; }
    for (auto& lc : lookups_c) { RP(t); lc[2] = t; }
    RP(random_c);
    const Fr y = rd.tr.squeeze_challenge();
    std::vector<int> h_c(vk->n_pieces);
    for (auto& c : h_c) { RP(t); c = t; }
    const Fr x = rd.tr.squeeze_challenge();
    std::vector<Fr> ev[3];
    ev[0].resize(vk->queries[0].size()); ev[1].resize(vk->queries[1].size()); ev[2].resize(vk->queries[2].size());
    for (auto& e : ev[0]) RS(e);
    for (auto& e : ev[1]) RS(e);
    Fr random_ev;
    RS(random_ev);
    std::vector<Fr> sigma_ev(vk->n_perm);
    for (auto& e : sigma_ev) RS(e);
    struct PermEv { Fr z, z_next, z_last; };
    std::vector<PermEv> perm_ev(vk->n_sets);
    for (uint32_t s = 0; s < vk->n_sets; s++) {
        RS(perm_ev[s].z); RS(perm_ev[s].z_next);
        if (s + 1 < vk->n_sets) RS(perm_ev[s].z_last);
    }
    struct LookupEv { Fr z, z_next, a, a_inv, s; };
    std::vector<LookupEv> lk_ev(vk->n_lookups);
    for (auto& e : lk_ev) { RS(e.z); RS(e.z_next); RS(e.a); RS(e.a_inv); RS(e.s); }

    const Fr one = Fr::one();
    const Fr xn = x.pow_u64(n);
    if (xn == one) return fail("the evaluation point lies in the domain");
    const Fr base = (xn - one) * Fr::from_u64(n).inv();                  // l_i(X) = (X^n - 1) / n * w^i / (X - w^i); (w^r x)^n = x^n
    // instance evaluations from the public values
    for (size_t q = 0; q < vk->queries[2].size(); q++) {
        const auto& vals = inst[vk->queries[2][q].first];
        const Fr xr = rotate(x, vk->queries[2][q].second);
        std::vector<Fr> den(vals.size()), wi(vals.size());
        Fr w = one;
        for (size_t i = 0; i < vals.size(); i++) { wi[i] = w; den[i] = xr - w; w = w * omega; }
        batch_invert(den);
        Fr acc = Fr::zero();
        for (size_t i = 0; i < vals.size(); i++) acc = acc + vals[i] * wi[i] * den[i];
        ev[2][q] = acc * base;
    }
    Fr l_0, l_last, l_blind = Fr::zero();
    {
        std::vector<Fr> wi, den;
        wi.push_back(one);
        Fr w = omega_inv.pow_u64(vk->bf + 1);                             // w^usable
        for (uint64_t i = u_rows; i < n; i++) { wi.push_back(w); w = w * omega; }
        for (auto& v : wi) den.push_back(x - v);
        batch_invert(den);
        l_0 = base * wi[0] * den[0];
        l_last = base * wi[1] * den[1];
        for (size_t i = 2; i < wi.size(); i++) l_blind = l_blind + base * wi[i] * den[i];
    }
    const Fr l_active = one - l_last - l_blind;
    // ---- the quotient's evaluation, folded with y in the prover's order
    Fr acc = plk_run_program(*vk, vk->gate_code, ev, y);
    if (vk->n_sets) {
        acc = acc * y + l_0 * (one - perm_ev[0].z);
        const Fr zl = perm_ev[vk->n_sets - 1].z;
        acc = acc * y + l_last * (zl * zl - zl);
        for (uint32_t s = 1; s < vk->n_sets; s++) acc = acc * y + l_0 * (perm_ev[s].z - perm_ev[s - 1].z_last);
        const Fr delta = Fr::from_u64(7).pow_u64(1ull << 28);             // Fr::DELTA
        for (uint32_t s = 0; s < vk->n_sets; s++) {
            Fr left = perm_ev[s].z_next, right = perm_ev[s].z;
            Fr cur = delta.pow_u64((uint64_t)s * vk->chunk_len) * beta * x;
            for (uint32_t j = s * vk->chunk_len; j < std::min(vk->n_perm, (s + 1) * vk->chunk_len); j++) {
                const Fr v = ev[vk->perm_cols[j].first][vk->perm_query[j]];
                left = left * (v + beta * sigma_ev[j] + gamma);
                right = right * (v + cur + gamma);
                cur = cur * delta;
            }
            acc = acc * y + (left - right) * l_active;
        }
    }
    for (uint32_t l = 0; l < vk->n_lookups; l++) {
        const LookupEv& e = lk_ev[l];
        const Fr a_in = plk_run_program(*vk, vk->lookups[l].in_code, ev, theta), s_in = plk_run_program(*vk, vk->lookups[l].tab_code, ev, theta);
        acc = acc * y + l_0 * (one - e.z);
        acc = acc * y + l_last * (e.z * e.z - e.z);
        acc = acc * y + (e.z_next * (e.a + beta) * (e.s + gamma) - e.z * (a_in + beta) * (s_in + gamma)) * l_active;
        acc = acc * y + l_0 * (e.a - e.s);
        acc = acc * y + (e.a - e.s) * (e.a - e.a_inv) * l_active;
    }
    const Fr h_eval = acc * (xn - one).inv();

    // ---- the opened commitments (plonk_openings.h: slots, query order, rotation sets).  A commitment is a list of (coefficient, point) parts: one
    // part for a point of the proof or the key, the quotient's pieces with the powers of x^n
    struct Part { int where; Fr coef; };                                   // where >= 0: proof point; < 0: key point -1 - where
    const PlkSlots sl(vk->n_advice, vk->n_sets, vk->n_lookups, vk->n_fixed, vk->n_perm);
    std::vector<std::vector<Part>> parts(sl.count);
    for (uint32_t c = 0; c < vk->n_advice; c++) parts[sl.advice + c] = {{advice_c[c], one}};
    for (uint32_t s = 0; s < vk->n_sets; s++) parts[sl.perm_z + s] = {{perm_c[s], one}};
    for (uint32_t l = 0; l < vk->n_lookups; l++) {
        parts[sl.lookup_z + l] = {{lookups_c[l][2], one}};
        parts[sl.lookup_a + l] = {{lookups_c[l][0], one}};
        parts[sl.lookup_s + l] = {{lookups_c[l][1], one}};
    }
    for (uint32_t c = 0; c < vk->n_fixed + vk->n_perm; c++) parts[sl.fixed + c] = {{-1 - (int)c, one}};
    { Fr pw = one; for (uint32_t i = 0; i < vk->n_pieces; i++) { parts[sl.h].push_back({h_c[i], pw}); pw = pw * xn; } }
    parts[sl.random] = {{random_c, one}};
    // the evaluation the proof claims for an opening
    auto claimed = [&](const PlkOpening& o) -> const Fr& {
        if (o.slot < sl.perm_z) return ev[0][o.query];
        if (o.slot < sl.lookup_z) { const PermEv& e = perm_ev[o.slot - sl.perm_z]; return o.rot == 0 ? e.z : (o.rot == 1 ? e.z_next : e.z_last); }
        if (o.slot < sl.lookup_a) { const LookupEv& e = lk_ev[o.slot - sl.lookup_z]; return o.rot == 0 ? e.z : e.z_next; }
        if (o.slot < sl.lookup_s) { const LookupEv& e = lk_ev[o.slot - sl.lookup_a]; return o.rot == 0 ? e.a : e.a_inv; }
        if (o.slot < sl.fixed) return lk_ev[o.slot - sl.lookup_s].s;
        if (o.slot < sl.sigma) return ev[1][o.query];
        if (o.slot < sl.h) return sigma_ev[o.slot - sl.sigma];
        return o.slot == sl.h ? h_eval : random_ev;
    };
    const std::vector<PlkOpening> queries = plk_opening_queries(sl, vk->queries[0], vk->queries[1], vk->bf, rotate, x);
    const PlkRotationSets plan(queries, sl.count);
    for (size_t q = 0; q < queries.size(); q++)
        if (claimed(queries[q]) != claimed(queries[plan.same[q]])) return fail("two different evaluations claimed for one (commitment, point)");

    // ---- SHPLONK
    const Fr sy = rd.tr.squeeze_challenge();
    const Fr sv = rd.tr.squeeze_challenge();
    RP(h1);
    const Fr su = rd.tr.squeeze_challenge();
    RP(h2);
#undef RP
#undef RS
    if (rd.pos != proof_len) return fail("trailing bytes in the proof");
    const std::vector<Fr>& all_points = plan.all_points;
    Fr zt = one;
    for (auto& pt : all_points) zt = zt * (su - pt);
    out.scalars.assign(pts.size(), Fr::zero());
    out.key_scalars.assign(vk->n_fixed + vk->n_perm + 1, Fr::zero());
    Fr outer_r = Fr::zero(), vi = one, z0 = one;
    std::vector<std::pair<uint32_t, Fr>> weights;                         // (slot, v^i z_i y^j)
    for (size_t si = 0; si < plan.sets.size(); si++) {
        const PlkRotationSets::Set& st = plan.sets[si];
        Fr zi = one;
        for (auto& pt : all_points) if (!plan.has(st.pts, pt)) zi = zi * (su - pt);
        if (si == 0) z0 = zi;
        // Lagrange basis of the set's points at u, shared by its commitments
        std::vector<Fr> lag(st.pts.size());
        for (size_t i = 0; i < st.pts.size(); i++) {
            Fr num = one, den = one;
            for (size_t j = 0; j < st.pts.size(); j++) if (j != i) { num = num * (su - st.pts[j]); den = den * (st.pts[i] - st.pts[j]); }
            lag[i] = num * den.inv();
        }
        const Fr scale = vi * zi;
        Fr inner_r = Fr::zero(), yj = one;
        for (size_t ci : st.coms) {
            Fr r_u = Fr::zero();
            for (size_t i = 0; i < lag.size(); i++) r_u = r_u + claimed(queries[plan.coms[ci].first[i]]) * lag[i];
            weights.push_back({plan.coms[ci].slot, scale * yj});
            inner_r = inner_r + yj * r_u;
            yj = yj * sy;
        }
        outer_r = outer_r + scale * inner_r;
        vi = vi * sv;
    }
    if (z0.is_zero()) return fail("u coincides with an opening point");
    // L = (sum_i v^i z_i (C_i - [r_i] G1) - [Z_T(u)] h1) / z_0;  the terms of L + u h2
    const Fr z0i = z0.inv();
    auto add_term = [&](int where, const Fr& s) {
        if (where >= 0) out.scalars[where] = out.scalars[where] + s;
        else out.key_scalars[-1 - where] = out.key_scalars[-1 - where] + s;
    };
    for (auto& w : weights) for (auto& part : parts[w.first]) add_term(part.where, w.second * part.coef * z0i);
    add_term(-1 - (int)(vk->n_fixed + vk->n_perm), (outer_r * z0i).neg());
    add_term(h1, (zt * z0i).neg());
    add_term(h2, su);
    out.h2 = pts[h2];
    return true;
}

// the MSM of `count` prepared proofs, proof b weighed by rho[b] (nullptr: one proof, weight 1): sum -> L + u h2, h2 sum -> second point
struct Msm { std::vector<uint64_t> points, scalars; };
void append(Msm& m, const uint64_t* pt, const Fr& s) {
    uint64_t w[4];
    s.to_words(w);
    m.points.insert(m.points.end(), pt, pt + 8);
    m.scalars.insert(m.scalars.end(), w, w + 4);
}

int32_t run_msm(gl355_ctx* ctx, const Msm& m, uint64_t out[8]) {
    const char* e = getenv("GL355_PLONK_VERIFY_DEVICE_MSM_MIN");
    const uint64_t min_terms = e ? strtoull(e, nullptr, 10) : PLONK_VERIFY_DEVICE_MSM_MIN;
    const uint64_t n = m.scalars.size() / 4;
    if (ctx && n >= min_terms) return gl355_bn254_g1_msm(ctx, m.points.data(), m.scalars.data(), n, out);
    bn254_g1_msm_host(m.points.data(), m.scalars.data(), n, out);
    return GL355_OK;
}

bool final_pairing(const gl355_plonk_vk* vk, const uint64_t lhs[8], const uint64_t h2_sum[8]) {
    uint64_t g1[16], g2[32];
    memcpy(g1, lhs, 64);
    bn254_g1_neg_host(h2_sum, g1 + 8);
    memcpy(g2, BN254_G2_GENERATOR, 128);
    memcpy(g2 + 16, vk->s_g2, 128);
    return bn254_pairing_product_is_one(g1, g2, 2);
}

// one proof, everything on the host
bool verify_one(const gl355_plonk_vk* vk, const uint64_t* instances, const uint32_t* lens, const uint8_t* proof, uint64_t proof_len, const char** why) {
    const double t0 = now_ms();
    Prepared p;
    if (!prepare(vk, instances, lens, proof, proof_len, p, why)) return false;
    const double t1 = now_ms();
    Msm m;
    for (size_t i = 0; i < p.points.size(); i++) if (!p.scalars[i].is_zero()) append(m, p.points[i].data(), p.scalars[i]);
    for (size_t j = 0; j < p.key_scalars.size(); j++) append(m, vk->key_points.data() + 8 * j, p.key_scalars[j]);
    uint64_t lhs[8];
    bn254_g1_msm_host(m.points.data(), m.scalars.data(), m.scalars.size() / 4, lhs);
    const double t2 = now_ms();
    const bool ok = final_pairing(vk, lhs, p.h2.data());
    g_stage_ms[0] = t1 - t0; g_stage_ms[1] = t2 - t1; g_stage_ms[2] = now_ms() - t2;
    if (!ok) *why = "SHPLONK opening check failed (pairing)";
    return ok;
}

// public values are canonical integers like every scalar of the ABI: the first of `count` that is not below r, or count
uint64_t first_noncanonical(const uint64_t* v, uint64_t count) {
    for (uint64_t i = 0; i < count; i++) if (Fr::geq_m(v + 4 * i)) return i;
    return count;
}
void clear_stage_ms() { g_stage_ms[0] = g_stage_ms[1] = g_stage_ms[2] = 0; }

bool all_zero(const uint64_t* p, int n) { uint64_t o = 0; for (int i = 0; i < n; i++) o |= p[i]; return o == 0; }

// 128-bit integers from ChaCha20 under `seed`: element i = the first 16 bytes of block i (32-bit counter i, nonce (stream, 0, i >> 32))
void random_u128(const uint8_t seed[32], uint32_t stream, uint64_t first, uint64_t count, uint64_t* out /* count x 4 */) {
    const BlindKey key = blind_key_from_bytes(seed);
    for (uint64_t i = 0; i < count; i++) {
        uint32_t o[16];
        chacha20_block(key, (uint32_t)(first + i), stream, 0, (uint32_t)((first + i) >> 32), o);
        out[4 * i] = (uint64_t)o[0] | ((uint64_t)o[1] << 32);
        out[4 * i + 1] = (uint64_t)o[2] | ((uint64_t)o[3] << 32);
        out[4 * i + 2] = out[4 * i + 3] = 0;
    }
}
// every point canonical and on the curve (the identity passes), on up to 16 threads: 2^23 points are ~2 s of one core
bool all_valid(const uint64_t* pts, uint64_t n) {
    const uint32_t n_threads = (uint32_t)std::min<uint64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), n / 4096 + 1);
    std::atomic<bool> good(true);
    auto work = [&](uint32_t t) {
        for (uint64_t i = n * t / n_threads; i < n * (t + 1) / n_threads && good.load(std::memory_order_relaxed); i++)
            if (!bn254_g1_valid_host(pts + 8 * i)) good = false;
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& t : pool) t.join();
    return good;
}
bool seed_or_random(const uint8_t* seed, uint8_t out[32]) {
    if (seed) { memcpy(out, seed, 32); return true; }
    return getrandom(out, 32, 0) == 32;
}

}  // namespace

extern "C" {

const char* gl355_plonk_verify_last_error(void) { return g_error.c_str(); }

int32_t gl355_plonk_verify_stage_ms(double ms[3]) {
    if (!ms) return GL355_E_INVALID_ARG;
    for (int i = 0; i < 3; i++) ms[i] = g_stage_ms[i];
    return GL355_OK;
}

int32_t gl355_plonk_vk_destroy(gl355_plonk_vk* vk) {
    delete vk;
    return GL355_OK;
}

int32_t gl355_plonk_vk_create(const uint64_t* desc, uint64_t words, const uint64_t* fixed_c, const uint64_t* sigma_c, const uint64_t digest[4], const uint64_t s_g2[16],
                              gl355_plonk_vk** out) {
    if (!desc || !s_g2 || !out || words < PLK_HDR) return bad_arg("plonk_vk_create: null or truncated argument");
    *out = nullptr;
    std::unique_ptr<gl355_plonk_vk> vk(new (std::nothrow) gl355_plonk_vk());
    if (!vk) return GL355_E_OOM;
    if (const char* what = plk_parse_desc(desc, words, PLK_MAX_K_VERIFIER, *vk)) { g_error = std::string("plonk_vk_create: ") + what; return GL355_E_INVALID_ARG; }
    if ((vk->n_fixed && !fixed_c) || (vk->n_perm && !sigma_c)) return bad_arg("plonk_vk_create: commitments missing");
    if (!plk_perm_queries(*vk, vk->perm_query)) return bad_arg("plonk_vk_create: a permutation column is not queried at the current rotation");
    // the key's points
    vk->key_points.assign(8ull * (vk->n_fixed + vk->n_perm + 1), 0);
    if (vk->n_fixed) memcpy(vk->key_points.data(), fixed_c, 64ull * vk->n_fixed);
    if (vk->n_perm) memcpy(vk->key_points.data() + 8ull * vk->n_fixed, sigma_c, 64ull * vk->n_perm);
    vk->key_points[8ull * (vk->n_fixed + vk->n_perm)] = 1;
    vk->key_points[8ull * (vk->n_fixed + vk->n_perm) + 4] = 2;
    for (uint32_t i = 0; i < vk->n_fixed + vk->n_perm; i++)
        if (!bn254_g1_valid_host(vk->key_points.data() + 8ull * i)) return bad_arg("plonk_vk_create: a commitment of the key is non-canonical or off the curve");
    if (const char* why = bn254_g2_invalid(s_g2, true)) { g_error = std::string("plonk_vk_create: s_g2: ") + why; return GL355_E_INVALID_ARG; }
    if (all_zero(s_g2, 16)) return bad_arg("plonk_vk_create: s_g2 is the identity");
    memcpy(vk->s_g2, s_g2, 128);
    // the transcript's initial scalar: as given, or what keygen takes (the header's, else the pinned-key rule)
    vk->digest = digest ? Fr::from_words(digest) : plk_pinned_digest(desc, words, fixed_c, sigma_c, *vk);
    *out = vk.release();
    return GL355_OK;
}

int32_t gl355_plonk_verify(gl355_ctx* ctx, const gl355_plonk_vk* vk, const uint64_t* instances, const uint32_t* lens, const uint8_t* proof, uint64_t proof_len, int32_t* ok) {
    (void)ctx;                                             // one proof stays on the host: its MSM is 1.4 of 5.8 ms, the pairing 4.0
    if (!vk || !ok || (!proof && proof_len) || (vk->n_instance && !lens)) return bad_arg("plonk_verify: null argument");
    *ok = 0;
    clear_stage_ms();
    uint64_t n_inst = 0;
    for (uint32_t c = 0; c < vk->n_instance; c++) n_inst += lens[c];
    if (n_inst && !instances) return bad_arg("plonk_verify: instance values missing");
    if (first_noncanonical(instances, n_inst) != n_inst) return bad_arg("plonk_verify: an instance value is not below r");
    const char* why = "";
    *ok = verify_one(vk, instances, lens, proof, proof_len, &why) ? 1 : 0;
    g_error = *ok ? "" : std::string("plonk_verify: ") + why;
    return GL355_OK;
}

int32_t gl355_plonk_verify_batch(gl355_ctx* ctx, const gl355_plonk_vk* vk, uint32_t n_proofs, const uint64_t* instances, const uint32_t* lens,
                                 const uint8_t* const* proofs, const uint64_t* proof_lens, const uint8_t seed[32], int32_t* ok, int32_t* first_bad) {
    if (!vk || !ok || (n_proofs && (!proofs || !proof_lens)) || (n_proofs && vk->n_instance && !lens)) return bad_arg("plonk_verify_batch: null argument");
    *ok = 0;
    if (first_bad) *first_bad = -1;
    clear_stage_ms();
    std::vector<uint64_t> inst_off(n_proofs + 1, 0);
    for (uint32_t b = 0; b < n_proofs; b++) {
        uint64_t cnt = 0;
        for (uint32_t c = 0; c < vk->n_instance; c++) cnt += lens[(size_t)b * vk->n_instance + c];
        if (cnt && !instances) return bad_arg("plonk_verify_batch: instance values missing");
        if (!proofs[b] && proof_lens[b]) return bad_arg("plonk_verify_batch: null proof");
        inst_off[b + 1] = inst_off[b] + cnt;
    }
    if (first_noncanonical(instances, inst_off[n_proofs]) != inst_off[n_proofs]) return bad_arg("plonk_verify_batch: an instance value is not below r");
    uint8_t key[32];
    if (!seed_or_random(seed, key)) return bad_arg("plonk_verify_batch: no seed given and getrandom failed");
    if (!n_proofs) { *ok = 1; g_error = ""; return GL355_OK; }
    const double t0 = now_ms();
    // per proof: transcript and scalar work, on at most 16 threads
    std::vector<Prepared> prep(n_proofs);
    std::vector<const char*> whys(n_proofs, nullptr);
    std::vector<uint8_t> good(n_proofs, 0);
    {
        std::atomic<uint32_t> next(0);
        auto work = [&]() {
            for (uint32_t b = next.fetch_add(1); b < n_proofs; b = next.fetch_add(1))
                good[b] = prepare(vk, instances ? instances + 4 * inst_off[b] : nullptr, lens + (size_t)b * vk->n_instance, proofs[b], proof_lens[b], prep[b], &whys[b]) ? 1 : 0;
        };
        const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
        const uint32_t n_threads = std::min(std::min(16u, hw), n_proofs);
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    for (uint32_t b = 0; b < n_proofs; b++) {
        if (good[b]) continue;
        if (first_bad) *first_bad = (int32_t)b;
        g_error = "plonk_verify_batch: proof " + std::to_string(b) + ": " + whys[b];
        return GL355_OK;
    }
    const double t1 = now_ms();
    // sum_b rho_b (L_b + u_b h2_b) as ONE multi-scalar multiplication (the key's points once, with their summed scalars), sum_b rho_b h2_b as a second
    std::vector<uint64_t> rho(4ull * n_proofs);
    random_u128(key, STREAM_BATCH_WEIGHTS, 0, n_proofs, rho.data());
    rho[0] = 1; rho[1] = 0;
    Msm big, h2s;
    std::vector<Fr> key_scalars(vk->n_fixed + vk->n_perm + 1, Fr::zero());
    for (uint32_t b = 0; b < n_proofs; b++) {
        const Fr w = Fr::from_words(rho.data() + 4 * b);
        for (size_t i = 0; i < prep[b].points.size(); i++) if (!prep[b].scalars[i].is_zero()) append(big, prep[b].points[i].data(), prep[b].scalars[i] * w);
        for (size_t j = 0; j < key_scalars.size(); j++) key_scalars[j] = key_scalars[j] + prep[b].key_scalars[j] * w;
        h2s.points.insert(h2s.points.end(), prep[b].h2.begin(), prep[b].h2.end());
        h2s.scalars.insert(h2s.scalars.end(), rho.begin() + 4 * b, rho.begin() + 4 * b + 4);
    }
    for (size_t j = 0; j < key_scalars.size(); j++) append(big, vk->key_points.data() + 8 * j, key_scalars[j]);
    uint64_t lhs[8], h2_sum[8];
    int32_t rc = run_msm(ctx, big, lhs);
    if (rc == GL355_OK) rc = run_msm(ctx, h2s, h2_sum);
    if (rc != GL355_OK) { g_error = "plonk_verify_batch: the device multi-scalar multiplication failed"; return rc; }
    const double t2 = now_ms();
    const bool pass = final_pairing(vk, lhs, h2_sum);
    g_stage_ms[0] = t1 - t0; g_stage_ms[1] = t2 - t1; g_stage_ms[2] = now_ms() - t2;
    if (pass) { *ok = 1; g_error = ""; return GL355_OK; }
    g_error = "plonk_verify_batch: the combined SHPLONK opening check failed (pairing)";
    if (first_bad) {
        for (uint32_t b = 0; b < n_proofs; b++) {
            const char* why = "";
            if (!verify_one(vk, instances ? instances + 4 * inst_off[b] : nullptr, lens + (size_t)b * vk->n_instance, proofs[b], proof_lens[b], &why)) {
                *first_bad = (int32_t)b;
                g_error = "plonk_verify_batch: proof " + std::to_string(b) + ": " + why;
                break;
            }
        }
    }
    return GL355_OK;
}

int32_t gl355_kzg_params_check(gl355_ctx* ctx, const uint64_t* g, uint64_t n_points, const uint64_t* g_lagrange, uint32_t log_n, const uint64_t s_g2[16],
                               const uint8_t seed[32], int32_t* ok) {
    if (!ctx || !g || !s_g2 || !ok || n_points < 1) return bad_arg("kzg_params_check: null argument or no points");
    *ok = 0;
    if (n_points > (1ull << 26) || (g_lagrange && (log_n > 26 || n_points < (1ull << log_n)))) return bad_arg("kzg_params_check: more than 2^26 points, or fewer than 2^log_n");
    uint8_t key[32];
    if (!seed_or_random(seed, key)) return bad_arg("kzg_params_check: no seed given and getrandom failed");
    auto reject = [&](const char* why) { g_error = std::string("kzg_params_check: ") + why; return GL355_OK; };
    if (bn254_g2_invalid(s_g2, true)) return reject("s_g2 is not a point of G2");
    if (all_zero(s_g2, 16)) return reject("s_g2 is the identity");
    if (all_zero(g, 8)) return reject("g[0] is the identity");
    if (!all_valid(g, n_points)) return reject("a point of g is non-canonical or off the curve");
    if (n_points > 1) {
        // powers: A = sum_{i<n-1} r_i g[i], B = sum_{i<n-1} r_i g[i+1] -- two scalar sets over the same bases, one call
        std::vector<uint64_t> sc(8ull * n_points, 0);
        random_u128(key, STREAM_PARAMS_POWERS, 0, n_points - 1, sc.data());
        memcpy(sc.data() + 4ull * n_points + 4, sc.data(), 32ull * (n_points - 1));
        uint64_t ab[16];
        const int32_t rc = gl355_bn254_g1_msm_batch(ctx, g, sc.data(), n_points, 2, ab);
        if (rc != GL355_OK) { g_error = "kzg_params_check: the multi-scalar multiplication failed"; return rc; }
        uint64_t g1[16], g2[32];
        memcpy(g1, ab + 8, 64);
        bn254_g1_neg_host(ab, g1 + 8);
        memcpy(g2, BN254_G2_GENERATOR, 128);
        memcpy(g2 + 16, s_g2, 128);
        if (!bn254_pairing_product_is_one(g1, g2, 2)) return reject("g is not a sequence of consecutive powers of the secret of s_g2");
    }
    if (g_lagrange) {
        const uint64_t n = 1ull << log_n;
        if (!all_valid(g_lagrange, n)) return reject("a point of g_lagrange is non-canonical or off the curve");
        std::vector<uint64_t> poly(4ull * n);
        random_u128(key, STREAM_PARAMS_LAGRANGE, 0, n, poly.data());
        uint64_t lhs[8], rhs[8];
        int32_t rc = gl355_bn254_g1_msm(ctx, g, poly.data(), n, lhs);
        if (rc == GL355_OK) rc = gl355_bn254_fr_ntt(ctx, poly.data(), log_n, 0);
        if (rc == GL355_OK) rc = gl355_bn254_g1_msm(ctx, g_lagrange, poly.data(), n, rhs);
        if (rc != GL355_OK) { g_error = "kzg_params_check: a device step of the Lagrange check failed"; return rc; }
        if (memcmp(lhs, rhs, 64) != 0) return reject("g_lagrange is not the Lagrange form of g");
    }
    *ok = 1;
    g_error = "";
    return GL355_OK;
}

}  // extern "C"
