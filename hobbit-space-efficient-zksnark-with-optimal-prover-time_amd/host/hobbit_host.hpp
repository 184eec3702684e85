// hobbit_host.hpp -- C++ host mirror of the reference's hot-path interface.
//
// The reference is one C++ executable whose "plugin API" for this path is a set of free functions
// and globals.  This header re-declares exactly those names with the reference's
// signatures so that a reference-shaped driver (src/main.cpp, test_PC) compiles against it
// unchanged; every body in hobbit_host.cpp is a thin call into the C ABI (include/hobbit_hip.h).
// Host-only pieces stay on the host exactly as in the reference: the libc rand()/random() draws
// (graphs, generate_randomness, queries) and the printf/exit self-check convention.
//
// Each declaration cites the reference declaration it mirrors.
#pragma once
#include <cstdint>
#include <cstddef>
#include <string>
#include <vector>
#include "hobbit_hip.h"
#include "hobbit_parity_lists.h"
#include "hobbit_whir.h"
#include "hobbit_brakingbase.h"
#include "hobbit_longcodes.h"
#include "hobbit_orion.h"
#include "hobbit_libcgen.h"
#include "hobbit_real.h"
#include "hobbit_elastic_real.h"
#include "hobbit_real_rs.h"

using std::vector;

namespace virgo {
// src/fieldElement.hpp:20-108 -- same 16-byte layout {real, img}, same operators; the arithmetic is
// the library's (canonical results identical to the reference's, see hobbit_field.hpp)
class fieldElement {
public:
    fieldElement() : real(0), img(0) {}
#ifdef HOBBIT_HOST_REFERENCE_BUILD
    // The reference declares these two (src/fieldElement.hpp:24,44): a user-provided copy constructor makes the class non-trivial for the
    // purposes of calls, so an F passed or returned by value travels through a hidden pointer instead of two registers.  The mirror must
    // agree with the reference's objects on that when both sit in one process (found the hard way: prove_multiplication_tree_stream_shallow
    // takes `F previous_r` by value).
    fieldElement(const fieldElement &b) : real(b.real), img(b.img) {}
    fieldElement &operator=(const fieldElement &b) { real = b.real; img = b.img; return *this; }
#endif
    fieldElement(long long x);
    fieldElement(long long x, long long y);
    fieldElement operator+(const fieldElement &o) const;
    fieldElement operator-(const fieldElement &o) const;
    fieldElement operator-() const;
    fieldElement operator*(const fieldElement &o) const;
    bool operator==(const fieldElement &o) const { return real == o.real && img == o.img; }
    bool operator!=(const fieldElement &o) const { return !(*this == o); }
    fieldElement &operator+=(const fieldElement &o) { *this = *this + o; return *this; }
    fieldElement &operator-=(const fieldElement &o) { *this = *this - o; return *this; }
    fieldElement &operator*=(const fieldElement &o) { *this = *this * o; return *this; }
    fieldElement inv() const;
    static fieldElement zero() { return fieldElement(0); }
    static fieldElement one() { return fieldElement(1); }
    unsigned long long real, img;
};
}  // namespace virgo
#define F virgo::fieldElement          /* src/config_pc.hpp:10-12 */
#define F_ONE virgo::fieldElement::one()
#define F_ZERO virgo::fieldElement::zero()

struct _hash { uint8_t arr[32]; };     /* src/Blake3_hash.h:3-5 */

/* globals that are part of the reference ABI (src/main.cpp:31,38; src/Our_PC.cpp:21; src/Elastic_PC.cpp:10,14) */
extern int tensor_row_size;
extern size_t BUFFER_SPACE;
extern bool linear_time;
extern int aggregation_queries;

/* src/polynomial.h:18-70 (coefficients highest degree first) */
class linear_poly { public: F a, b; linear_poly() {} linear_poly(const F &aa, const F &bb) : a(aa), b(bb) {} F eval(const F &x) const { return a * x + b; } };
class quadratic_poly { public: F a, b, c; quadratic_poly() {} quadratic_poly(const F &aa, const F &bb, const F &cc) : a(aa), b(bb), c(cc) {}
    F eval(const F &x) const { return ((a * x) + b) * x + c; } };
class cubic_poly { public: F a, b, c, d; cubic_poly() {} cubic_poly(const F &aa, const F &bb, const F &cc, const F &dd) : a(aa), b(bb), c(cc), d(dd) {}
    F eval(const F &x) const { return (((a * x) + b) * x + c) * x + d; } };

/* src/sumcheck.h:21-43 (the members the hot-path functions fill) */
#ifndef HOBBIT_HOST_REFERENCE_BUILD
struct proof {
    int type = 0;
    vector<vector<F>> randomness;
    vector<quadratic_poly> q_poly;
    vector<cubic_poly> c_poly;
    vector<F> vr;
    F final_rand;
};
#else
/* in front of the reference's own objects a `proof` (and the mul_tree_proof that holds a vector of them) is returned BY VALUE into storage
 * the reference's code laid out and will destroy: every member of src/sumcheck.h:21-43, in its order */
struct proof {
    int type = 0;
    vector<vector<F>> randomness;
    vector<quadratic_poly> q_poly;
    vector<cubic_poly> c_poly;
    vector<F> output;
    vector<F> vr;
    vector<F> gr;
    vector<F> liu_sum;
    vector<vector<F>> sig;
    vector<vector<F>> final_claims_v;
    F divident, divisor, quotient, remainder;
    vector<vector<vector<F>>> w_hashes;
    vector<F> r, individual_sums;
    vector<vector<F>> Partial_sums;
    vector<quadratic_poly> q_poly1;
    vector<quadratic_poly> q_poly2;
    F final_rand;
    F final_sum;
    int K = 0;
};
#endif

/* src/expanders.h:7-16 */
class graph {
public:
    int degree = 0;
    vector<vector<long long>> neighbor, r_neighbor;
    vector<vector<F>> weight, r_weight;
    long long L = 0, R = 0;
};
extern graph _C[100], D[100];                                   /* src/expander.cpp:2 */

/* device context used by every call below; created on first use on HOBBIT_DEVICE (default 0).
 * Creation failure (no GPU / library) prints the reason and exits(-1), the reference's own error
 * convention -- there is no CPU fallback. */
hobbit_ctx *hobbit_host_ctx();
void hobbit_host_shutdown();

/* src/mimc.h:5-6 */
void init_hash();
F mimc_hash(F input, F k);
/* src/utils.hpp:13,18,23,39,57 */
void precompute_beta(vector<F> r, vector<F> &B);
vector<F> generate_randomness(int size);
F evaluate_vector(vector<F> v, vector<F> r);
void fft(vector<F> &arr, int logn, bool flag);
void _fft(F *arr, int logn, bool flag);
/* src/expanders.h:78 ; src/linear_code_encode.h:62 */
long long expander_init_store(long long n, int dep = 0);
void hobbit_host_upload_graphs(long long n);                    /* device upload of the graphs already in _C / D (drawn by another copy of expander_init_store) */
int encode_monolithic(const F *src, F *dst, long long n, int dep = 0);
/* src/Blake3_hash.h:9 */
void blake3_hash(uint8_t *src, uint8_t *dst);
/* src/merkle_tree.h:25,33,36,38 */
namespace merkle_tree {
_hash hash_double_field_element_merkle_damgard_blake(virgo::fieldElement x, virgo::fieldElement y, virgo::fieldElement z, virgo::fieldElement w, _hash &prev_hash);
namespace merkle_tree_prover {
void MT_commit_Blake(F *leafs, vector<vector<_hash>> &hashes, int N);
void create_tree_blake(int ele_num, vector<vector<_hash>> &hashes, const int element_size = 256 / 8, bool alloc_required = false);
vector<_hash> open_tree_blake(vector<vector<_hash>> &MT_hashes, vector<size_t> c, int collumns);
}  // namespace merkle_tree_prover
}  // namespace merkle_tree
/* src/PC_utils.h:6 */
void compute_tensorcode(vector<F> &message, vector<vector<F>> &tensor);
/* src/Our_PC.hpp:11-15 */
void commit_standard(vector<F> &poly, _hash &comm, vector<vector<_hash>> &MT_hashes, vector<vector<vector<F>>> &_tensor, int K);
void test_PC(size_t N, int option, int K);                                          /* options 4, 1 and 3 (Brakedown) */
/* Base-field polynomials (include/hobbit_real.h): commit_standard / open_standard (linear_time, tensor_row_size set as for commit_standard) for a
 * polynomial that lives on the device as N reals of 8 bytes.  commit_standard_real takes the device buffer (from hobbit_malloc) over and makes a
 * half commitment; open_standard_real opens it.  test_PC_real is test_PC's option 4 with the polynomial drawn on the device as reals
 * (`host/test_pc real <logN> <K>`): the same libc draws in the same order, the same root and Ps. */
void commit_standard_real(uint64_t *d_poly, size_t N, vector<vector<_hash>> &MT_hashes, int K);
void open_standard_real(size_t N, vector<F> x, vector<vector<_hash>> &Commitment_MT, int K, double &vt, double &ps);
void test_PC_real(size_t N, int K);
/* test_PC's option 1 (RS x RS, tensor_row_size 128) the same way (include/hobbit_real_rs.h): commit_standard_real / open_standard_real route to the
 * RS x RS calls when linear_time is false. */
void test_PC_real_rs(size_t N, int K);
/* src/Our_PC.hpp: the Brakedown comparison baseline (src/Our_PC.cpp:197-236, 432-520).  commit_standard_brakedown draws the row code's graphs
 * (expander_init_store(B)) and keeps the encoded matrix on the device; open_brakedown_standard draws r (rows x random()) and the 2900 columns
 * (rand() % 2B), opens, and prints the reference's "PC Open: pt = .., ps = .. KB, vt = .. sec" line. */
void commit_standard_brakedown(vector<F> &poly, _hash &comm, vector<vector<_hash>> &MT_hashes);
void open_brakedown_standard(vector<F> &poly, vector<F> x, vector<vector<_hash>> &Commitment_MT);
/* the messages of the last open_brakedown_standard (the reference returns none); ps as printed, from 0 (the reference's `double ps;` is
 * uninitialised, src/Our_PC.cpp:508) */
struct hobbit_host_brakedown_transcript { vector<F> r, aggr_beta, aggr_r, reply; vector<uint64_t> I; vector<uint8_t> paths; double ps = 0, pt = 0, vt = 0; };
hobbit_host_brakedown_transcript &hobbit_host_last_brakedown();
void open_standard(vector<F> &poly, vector<F> x, vector<vector<_hash>> &Commitment_MT, vector<vector<vector<F>>> &_tensor, int K, double &vt, double &ps);
/* The reference's open_standard returns nothing but vt / ps (it never serialises its proof); the messages the device prover
 * produced for the last open_standard call are kept here.  Layouts as hobbit_open_out / hobbit_shockwave_out (include/hobbit_hip.h). */
struct hobbit_host_shockwave_transcript {
    vector<uint32_t> I; vector<F> q1, r1, vr1, q2, r2, vr2, wq, wa, wscal, reply, wqreply, wfinal; F fin1, fin2;
    vector<uint8_t> wroots, paths, wqpaths; uint8_t whir_root[32]; vector<int32_t> wqidx, wqn; int wchecks[2] = {0, 0}, iters = 0;
};
struct hobbit_host_open_transcript {
    int queries = 0, rounds = 0;
    vector<uint32_t> cols, rows; vector<F> reply, qpoly, r, vr, fin, scalars; vector<uint8_t> paths; uint8_t roots[64];
    int checks[3] = {0, 0, 0};
    hobbit_host_shockwave_transcript sp_c, sp_f;
};
hobbit_host_open_transcript &hobbit_host_last_open();
/* src/Our_PC.cpp:258-272, 291-305 (file-local helpers of open_standard) */
void _aggregate_axpy(vector<F> &poly, vector<F> beta1, vector<F> &aggregated_vector, int K);
void _compute_aggregation_reply(vector<vector<size_t>> &I, vector<vector<F>> &reply, vector<vector<vector<F>>> &_tensor, int K);
/* src/sumcheck.h:70,78 */
struct proof generate_2product_sumcheck_proof(vector<F> &_v1, vector<F> &_v2, F previous_r, double &vt, double &ps);
struct proof _generate_3product_sumcheck_proof(vector<F> &v1, vector<F> &v2, vector<F> &v3, F previous_r, double &vt, double &ps);

/* src/sumcheck.h:89 (src/sumcheck.cpp:434-501).  The reference folds its four inputs in place and returns nothing; here element 0 of
 * arr_L, arr_R, arr_O, add_gate is set to the fully folded value (all a caller can use) and the rest is left as passed in. */
void prove_gate_consistency_standard(vector<F> &arr_L, vector<F> &arr_R, vector<F> &arr_O, vector<F> &add_gate, vector<F> r, double &vt, double &ps);
/* src/sumcheck.h:67,74,78,81 ; src/utils.hpp:24,41 */
int evaluate_parity_matrix(vector<F> &A, vector<F> &beta1, int Offset, int n, int dep, int &lvl);
proof prove_linear_code(vector<F> &codeword, int n, double &vt, double &ps);
struct proof prove_fft(vector<F> &m, vector<F> r, F previous_sum, double &vt, double &ps);
struct proof prove_fft_matrix(vector<vector<F>> M, vector<F> r, F previous_sum, double &vt, double &ps);
void phiGInit(vector<F> &phi_g, const vector<F>::const_iterator &rx, const F &scale, int n, bool isIFFT);
vector<F> prepare_matrix(vector<vector<F>> M, vector<F> r);
vector<vector<F>> transpose(vector<vector<F>> M);

/* src/sumcheck.h:8-20 */
struct mul_tree_proof {
    F initial_randomness;
    size_t size = 0;
    F in1, in2;
    F out_eval;
    vector<struct proof> proofs;
    vector<F> output;
    vector<F> final_r;
    vector<F> global_randomness, individual_randomness;
    vector<F> partial_eval;
    F final_eval;
};
/* src/sumcheck.h:92, src/sumcheck.cpp:275 (defined there without a header declaration) */
mul_tree_proof prove_multiplication_tree_new(vector<vector<F>> &input, F previous_r, vector<F> prev_x, double &vt, double &ps);
struct proof batch_3product_sumcheck(vector<vector<F>> &arr1, vector<vector<F>> &arr2, vector<vector<F>> &arr3, vector<F> a, double &vt, double &ps);
/* src/PC_utils.h:9 : tensor = 2*tensor_row_size row pointers of 2*size/tensor_row_size F each */
void _compute_tensorcode(F *message, F **tensor, int size);
/* src/Virgo.h:27-47, 95 ; src/Virgo.cpp:120, 435.  The encoded matrix and the column tree stay on the device (d_*); matrix /
 * encoded_matrix are materialised on the host as the reference has them (k rows). */
struct shockwave_data {
    int k = 0;
    int N = 0;
    F **encoded_matrix = nullptr, **matrix = nullptr;
    vector<vector<_hash>> MT;
    void *d_matrix = nullptr, *d_enc = nullptr, *d_levels = nullptr;      /* not in the reference: device residents of the same data */
    ~shockwave_data();
};
shockwave_data *shockwave_commit(vector<F> &poly, int k);
void shockwave_prove(shockwave_data *data, vector<F> x, double &vt, double &ps);
struct hobbit_host_shockwave_transcript;
hobbit_host_shockwave_transcript &hobbit_host_last_shockwave();           /* the messages of the last shockwave_prove (the reference returns none) */
/* src/Virgo.h:52-60, src/Virgo.cpp:160-178, 519-686: the standalone WHIR baseline (test_PC's last branch, src/Our_PC.cpp:843-859), on the
 * device through hobbit_whir_commit / hobbit_whir_prove_any (include/hobbit_whir.h), 2^9 <= N <= 2^26.  whir_commit keeps the polynomial, the
 * regrouped codeword and the tree on the device (d_poly, d_com, d_levels); MT is read back, poly_com and the FRI members stay empty on the
 * host.  _whir_prove draws from libc in the reference's order, exits on the reference's two checks and accumulates ps as the reference does.
 * Left out of the build that sits in front of the reference's objects: there a caller's Whir_data has the reference's layout. */
#ifndef HOBBIT_HOST_REFERENCE_BUILD
struct Whir_data {
    int k = 0;
    vector<F> poly, poly_com;
    vector<vector<_hash>> MT;
    vector<vector<vector<_hash>>> FRI_MT;
    vector<vector<F>> FRI_poly;
    void *d_poly = nullptr, *d_com = nullptr, *d_levels = nullptr;         /* not in the reference: device residents of the same data */
    Whir_data() = default;
    Whir_data(const Whir_data &) = delete;
    Whir_data &operator=(const Whir_data &) = delete;
    ~Whir_data();
};
void whir_commit(vector<F> &poly, Whir_data &data);
void _whir_prove(Whir_data &data, vector<F> x, double &vt, double &ps);
/* the messages of the last _whir_prove (the reference returns none); layouts as hobbit_whir_out */
struct hobbit_host_whir_transcript {
    vector<F> qpoly, a, scal, qreply, final_pb; vector<uint8_t> fri_roots, qpaths; vector<int32_t> qidx, qn; int checks[2] = {0, 0}, iters = 0;
    double ps = 0, vt = 0;
};
hobbit_host_whir_transcript &hobbit_host_last_whir();
void test_whir(size_t N);                                                 /* test_PC's last branch; `host/test_pc whir <logN>` */
#endif
/* src/Our_PC.cpp:114-144, 238-256, 355-429, 827-842 ; src/PC_utils.cpp:389-394: the Braking base comparison baseline (test_PC option 5), on the
 * device through include/hobbit_brakingbase.h.  tensor_row_size is the row length (N / K) and expander_init_store(tensor_row_size) has run, as
 * in the reference's driver.  commit_brakingbase prints the reference's "%d,%d" line and keeps the encoded matrix on the device;
 * open_brakingbase is one hobbit_brakingbase_open (libc draws in the reference's order), exits on the reference's checks and prints its
 * "Ps : .., Vt : .." line; the verifier emulation behind it is reduced to its proof-size accounting.  _aggregate_brakingbase and
 * recursive_prover_brakingbase are the reference's two steps over this mirror's own entry points (host vectors in, C_c set / consumed).
 * test_PC itself keeps refusing option 5: the driver is test_brakingbase, reached as `host/test_pc brakingbase <logN> <K>`; a shape the
 * library does not serve prints an error and exits with -1 before anything is drawn.
 * Left out of the build that sits in front of the reference's objects, which has the reference's own. */
#ifndef HOBBIT_HOST_REFERENCE_BUILD
void commit_brakingbase(vector<F> &poly, vector<vector<_hash>> &MT_hashes);
void _aggregate_brakingbase(vector<F> &poly, vector<F> beta1, vector<F> random_points, vector<F> &codeword);
void open_brakingbase(vector<F> &poly, vector<F> x, vector<vector<_hash>> &MT_hashes);
void recursive_prover_brakingbase(vector<F> &codeword, vector<size_t> I, double &vt, double &ps);
/* the messages of the last open_brakingbase (the reference returns none); layouts as hobbit_brakingbase_open_out */
struct hobbit_host_brakingbase_transcript {
    vector<uint32_t> I; vector<F> reply, aggr, p1_q, p1_r, p1_r1; F p1_vr[2], p1_fin; vector<uint8_t> paths; uint8_t cc_root[32], cp_root[32];
    hobbit_host_shockwave_transcript sp_c; double stage_ms[6] = {0, 0, 0, 0, 0, 0}, ps = 0, vt = 0;
};
hobbit_host_brakingbase_transcript &hobbit_host_last_brakingbase();       /* the parity part: hobbit_host_last_parity_open() */
void test_brakingbase(size_t N, int K);
/* the long forms (include/hobbit_longcodes.h): the same three with 128 <= N / K <= 2^21, reached as `host/test_pc brakingbase_any <logN> <K>`;
 * test_brakingbase_any also prints the opening's six stage times ("stage_ms ...") */
void commit_brakingbase_any(vector<F> &poly, vector<vector<_hash>> &MT_hashes);
void open_brakingbase_any(vector<F> &poly, vector<F> x, vector<vector<_hash>> &MT_hashes);
void test_brakingbase_any(size_t N, int K);
#endif
/* src/Our_PC.cpp:28-65, 173-195, 523-602, 780-793 ; src/PC_utils.cpp:150-166: the Orion comparison baseline (test_PC option 2), on the device
 * through include/hobbit_orion.h.  commit_standard_orion draws the graphs of n = sqrt(N) as the reference does, prints its "OK" line and keeps
 * the tensor AND its tree on the device (the tree has N leaves: 16 GB of levels at 2^28); MT_hashes gets the level count and the root.
 * open_orion_standard is one hobbit_orion_open (libc draws in the reference's order) without the Q^2 opening paths -- the reference only
 * counts them, and this mirror never materialises them on the host -- then hobbit_orion_proof_size; it exits on the reference's checks and
 * prints its " ps = .., vt = .." line.  recursive_prover_orion is the reference's sequence over this mirror's own entry points (host vectors
 * in); _compute_tensorcode_linear_code returns the square tensor of a host message.  test_PC itself keeps refusing option 2: the driver is
 * test_orion, reached as `host/test_pc orion <logN>`; a shape the library does not serve prints an error and exits with -1 before anything is
 * drawn.  Left out of the build that sits in front of the reference's objects, which has the reference's own. */
#ifndef HOBBIT_HOST_REFERENCE_BUILD
void _compute_tensorcode_linear_code(vector<F> &message, vector<vector<F>> &tensor);
void commit_standard_orion(vector<F> &poly, _hash &comm, vector<vector<_hash>> &MT_hashes);
void open_orion_standard(vector<F> &poly, vector<F> x, vector<vector<_hash>> &Commitment_MT);
void recursive_prover_orion(vector<vector<F>> &codewords, double &vt, double &ps);
/* the messages of the last open_orion_standard (the reference returns none); layouts as hobbit_orion_open_out */
struct hobbit_host_orion_transcript {
    vector<uint32_t> I, J; vector<F> p1_q, p1_r, p1_r1, p1_r2; F p1_vr[2], p1_fin; uint8_t c_root[32], cp_root[32];
    hobbit_host_shockwave_transcript sp_c; double stage_ms[6] = {0, 0, 0, 0, 0, 0}, ps = 0, vt = 0;
};
hobbit_host_orion_transcript &hobbit_host_last_orion();                   /* the parity part: hobbit_host_last_parity_open() */
void test_orion(size_t N);
#endif
/* src/PC_utils.cpp:6-7 ; src/linear_code_encode.cpp:3-4 ; src/sumcheck.cpp:27,29 : globals of the reference ABI.  C_f / C_c are set by
 * this mirror's shockwave users as the reference's _aggregate / aggregate do; scratch / __encode_initialized exist for source
 * compatibility only (the device encode has no host scratch); routine_time accumulates the time spent re-generating streams, sc_vt is
 * never written on the prover side. */
extern shockwave_data *C_f, *C_c;
/* src/sumcheck.cpp:25, 2671, 2708, 3201 (defined there without header declarations): the succinct opening of the code's parity matrix.
 * commit_parity_matrix(n) needs expander_init_store(n) and sets the global C_p (N = 8P, k = 16, the column tree; the matrix and its encoded
 * rows stay on the device, matrix / encoded_matrix are null).  open_parity_matrix draws from libc in the reference's order, exits on the
 * reference's "Error 1" / "Error 2", accumulates ps piece by piece and, like the reference (shockwave_prove deletes its argument), leaves C_p
 * deleted.  Index padding is 0 (include/hobbit_parity.h).  prove_linear_code_batch draws r1, r2 itself; a power-of-two number of codewords. */
extern shockwave_data *C_p;
void commit_parity_matrix(int n);
void open_parity_matrix(vector<F> r1, vector<F> r2, int n, double &vt, double &ps);
proof prove_linear_code_batch(vector<vector<F>> &codewords, int n, double &vt, double &ps);
/* the messages of the last open_parity_matrix (the reference returns none); layouts as hobbit_parity_open_out */
struct hobbit_host_parity_transcript {
    struct tree { vector<F> cpoly, r, vr, fin, final_r; F evals[2]; int layers = 0; };
    int n = 0; size_t P = 0;
    tree t1, t2;
    vector<F> p2, p2_r, p3, p3_r, p4, p4_r; F p2_vr[3], p3_vr[2], p4_vr[2], p2_fin, p3_fin, p4_fin;
    uint8_t cw_root[32]; F scalars[4], partial[7], acc_y[2]; int checks[2] = {0, 0};
    hobbit_host_shockwave_transcript sp_p, sp_w;
};
hobbit_host_parity_transcript &hobbit_host_last_parity_open();
extern F *scratch[2][100];
extern bool __encode_initialized;
extern double routine_time, sc_vt;

/* src/witness_stream.h:5-16 (the fields the PCS reads), src/Elastic_PC.hpp:12-16 */
struct stream_descriptor {
    int idx = 0, offset = 0, stage = 0;
    bool finished = false;
    size_t pos = 0, pos_j = 0;
    size_t data_size = 0, row_size = 0, col_size = 0, size = 0, layer = 0, tree_pos = 0;
    std::string name;
    size_t input_pos = 0, input_pos_j = 0, input_data_size = 0, input_size = 0;
    std::string input_name;
};
void read_stream_PC(stream_descriptor &fd, F *v, int size);      /* synthetic default stream only (src/witness_stream.cpp:2405-2411) */
void commit(stream_descriptor fd, _hash &comm, vector<vector<_hash>> &MT_hashes);
void init_commitment(bool mod);
void read_stream(stream_descriptor &fd, vector<F> &v, int size);  /* default branch only (src/witness_stream.cpp:2348-2352) */
void open(stream_descriptor fd, vector<F> x, vector<vector<_hash>> &Commitment_MT, double &vt, double &ps);   /* !linear_time (RS x RS) */
/* src/main.cpp:985-1087: the non-streaming prover.  Everything it proves runs on the device (both commit_standard / open_standard modes,
 * prove_multiplication_tree_new, prove_gate_consistency_standard); what it READS comes from the witness generator
 * (read_trace, src/witness_stream.cpp:1701; read_memory), which is not part of this library: a reference build assigns its own two
 * functions to the hooks, a test assigns synthetic readers.  circuit_size: src/main.cpp global (set by init_stream, :1100). */
extern size_t circuit_size;
extern void (*hobbit_read_trace_hook)(stream_descriptor &fd, vector<F> &buff_L, vector<F> &buff_R, vector<F> &buff_O, vector<int> &buff_S);
extern void (*hobbit_read_memory_hook)(stream_descriptor &fd, vector<F> &buff_addr, vector<F> &buff_value, vector<F> &buff_access);
void reset_stream(stream_descriptor &fd);                      /* src/witness_stream.cpp:228-234 */
/* src/sumcheck.h:90-91, src/sumcheck.cpp:796 / :503: the streaming gate-consistency provers.  The trace is read through
 * hobbit_read_trace_hook (BUFFER_SPACE gates per call); has_lookups / lookup_rand: src/main.cpp:70 / :67 (prove_gate_consistency_lookups
 * reads lookup_rand[0..1] and needs has_lookups set, as compute{3,4}p_error_terms do in the reference). */
extern bool has_lookups;
extern vector<F> lookup_rand;
extern int tensor_code;                                        /* src/Elastic_PC.cpp:14 (1 = the tensor code; the only value the device path implements) */
void prove_gate_consistency(stream_descriptor tr, vector<F> r, double &vt, double &ps);
void prove_gate_consistency_lookups(stream_descriptor tr, vector<F> r, double &vt, double &ps);
/* the messages of the last streaming gate prover (the reference returns none): layouts as hobbit_gate_stream_out / hobbit_gate_lkp_stream_out */
struct hobbit_host_gate_transcript { vector<F> R, a, poly, gr, fin, Peval, b, q2, r2, vr2; F fin2; int checks[5] = {0, 0, 0, 0, 0}; bool lookups = false; };
hobbit_host_gate_transcript &hobbit_host_last_gate();
void test_Elastic_PC(size_t N, int option);                     /* src/Elastic_PC.cpp:736-808: options 1, 2 and 3 (the streaming Brakedown baseline: sets BUFFER_SPACE itself) */
/* src/Elastic_PC.cpp:112-172, 287-313, 561-623: the streaming Brakedown baseline.  The stream is read on the host (read_stream_PC, descriptor
 * by value: three passes); the device keeps one group of four chunks.  open_brakedown_stream draws r_v[0] (generate_randomness(1)) and the
 * 2935 indices (rand() % 2B) and prints the reference's "Ps : .., Vt : .." line; its verifier side is restated as proof-size accounting only. */
void commit_brakedown_stream(stream_descriptor fd, vector<vector<_hash>> &MT_hashes);
void aggregate_brakedown(stream_descriptor fd, vector<F> beta1, vector<F> random_points, vector<F> &aggregated_vector1, vector<F> &aggregated_vector2);
void compute_reply(stream_descriptor fd, vector<size_t> I, vector<vector<F>> &R);
void open_brakedown_stream(stream_descriptor fd, vector<F> x, vector<vector<_hash>> &Commitment_MT);
/* the messages of the last open_brakedown_stream (the reference returns none): reply is queries x chunks, paths queries x log2(2B) x 32 B */
struct hobbit_host_brakedown_stream_transcript { vector<F> beta, r_v, aggr_beta, aggr_r, reply; vector<uint64_t> I; vector<uint8_t> paths; double ps = 0, vt = 0; };
hobbit_host_brakedown_stream_transcript &hobbit_host_last_brakedown_stream();
/* the messages of the last Elastic open (the reference returns only vt / ps); layouts as hobbit_elastic_open_out */
struct hobbit_host_elastic_transcript {
    int queries = 0, rounds = 0, reply_len = 0, ncols = 0;
    vector<uint32_t> cols, rows; vector<F> reply, qpoly, r, vr, fin, rx; vector<uint8_t> paths; uint8_t cf_root[32]; F rv0;
    int checks[2] = {0, 0};
    hobbit_host_shockwave_transcript sp_f;
    /* Elastic_PC::open under linear_time (option 2; recursive_prover_Spielman_stream): remaining columns, padded size of aux_commit, C_c's root,
     * s[0] / s2 / y1, and shockwave_prove(C_c, .); qpoly / r then hold P1, P2, P3, P5 and checks[0] is prove_fft_matrix's test */
    bool lin = false; int nrem = 0; size_t np = 0; uint8_t cc_root[32]; vector<F> scal;
    hobbit_host_shockwave_transcript sp_c;
};
hobbit_host_elastic_transcript &hobbit_host_last_elastic_open();
/* On-wire form of an opening proof.  The reference never serialises a proof (struct proof / mul_tree_proof stay in
 * memory, src/sumcheck.h:8-43), so this layout is ours; little-endian throughout:
 *   header  "HBPF" | u32 version = 1 | u32 kind (1 = open_standard, RS x expander; 2 = RS x RS opening: open_standard with !linear_time or
 *           Elastic_PC::open) | u32 number of sections
 *   section u32 tag | u64 payload bytes | payload   (field elements as 16-byte {real, img}; hashes as 32 bytes; indices as u32 / i32)
 * The nested shockwave_prove transcripts are sections whose payload is itself a sequence of sections.  Unknown tags are skipped by the
 * reader, a truncated or malformed buffer is rejected.  A proof carries messages only -- no checks, no timings. */
std::vector<uint8_t> hobbit_host_serialize_open(const hobbit_host_open_transcript &t);
bool hobbit_host_deserialize_open(const uint8_t *buf, size_t n, hobbit_host_open_transcript &t);
std::vector<uint8_t> hobbit_host_serialize_rs_open(const hobbit_host_elastic_transcript &t);
bool hobbit_host_deserialize_rs_open(const uint8_t *buf, size_t n, hobbit_host_elastic_transcript &t);
/* Elastic_PC on base-field streams (include/hobbit_elastic_real.h): the real parts of the two default streams, 8 bytes per value, and commit /
 * open / test_Elastic_PC reading, uploading and pushing those (options 1 and 2).  test_Elastic_PC itself keeps widening, as test_PC does. */
void read_stream_PC_real(stream_descriptor &fd, uint64_t *v, int size);
void read_stream_real(stream_descriptor &fd, uint64_t *v, int size);
void commit_real(stream_descriptor fd, _hash &comm, vector<vector<_hash>> &MT_hashes);
void open_real(stream_descriptor fd, vector<F> x, vector<vector<_hash>> &Commitment_MT, double &vt, double &ps);
void test_Elastic_PC_real(size_t N, int option);
void test_Elastic_PC_commit(size_t N, int option);              /* commit phase of test_Elastic_PC (src/Elastic_PC.cpp:736-771) */
/* src/sumcheck.h:84, src/sumcheck.cpp:1150 : the streaming multiplication-tree prover over read_stream (default stream only) */
vector<F> prove_multiplication_tree_stream_shallow(stream_descriptor fd, int vectors, int size, F previous_r, int distance, vector<F> prev_x, bool naive, double &vt, double &ps);
/* src/sumcheck.cpp:983-1011: Elastic_PC commitments to / openings of the "PC_layer" streams of the batched path */
void commit_layers(stream_descriptor fd, vector<stream_descriptor> &fd_com, vector<vector<vector<_hash>>> &MT_hashes, int batches, int layer_id, int distance);
void open_layers(vector<stream_descriptor> &fd_com, vector<vector<vector<_hash>>> &MT_hashes, double &vt, double &ps);
void generate_3product_sumcheck_beta_stream_batch_optimized(stream_descriptor fd, vector<vector<F>> r, int batches, int distance, int layer_id, vector<F> old_claims,
                                                            vector<F> &new_claims, vector<vector<F>> &new_r, double &vt, double &ps);

/* Not in the reference: the 16 GiB `_tensor` of a 2^28 commit stays on the device.
 * commit_standard leaves `_tensor[i]` empty unless HOBBIT_MATERIALIZE_TENSOR=1 (or the tensor is
 * under 256 MiB); the device-resident commitment of the last commit_standard is reachable here
 * and is what _compute_aggregation_reply / open_tree_blake read when `_tensor[i]` is empty. */
hobbit_commitment *hobbit_host_last_commitment();
void hobbit_host_materialize_tensor(vector<vector<vector<F>>> &_tensor);
