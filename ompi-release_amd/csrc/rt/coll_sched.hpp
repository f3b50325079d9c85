// coll_sched.hpp -- schedule compiler of coll/mi355x.
//
// The reference's per-element result is fixed by the order in which its point-to-point
// schedule applies ompi_op_reduce(op, source, target) (target = target (op) source,
// ompi/op/op.h:540-574).  This compiler re-runs each schedule of coll/tuned SYMBOLICALLY --
// buffers hold expression ids instead of data -- and turns the resulting expression tree into a
// device program: a left fold (k_fold) when the tree is a chain, a register program (k_tree)
// otherwise.  The device then evaluates that exact tree per element, reading every rank's input
// over xGMI, so float results match the reference's schedule bit for bit without moving data
// the way the reference does.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "coll_internal.hpp"

namespace mi355x {

struct Expr {
    int rank;       // >= 0: leaf (that rank's input); -1: op node
    int out, in;    // op node: op2(out = pool[out], in = pool[in])
};

struct ExprPool {
    std::vector<Expr> e;
    int leaf(int r) { e.push_back({r, -1, -1}); return (int)e.size() - 1; }
    int op(int out, int in) { e.push_back({-1, out, in}); return (int)e.size() - 1; }
};

// A compiled per-element program.
struct Program {
    bool is_fold = false;
    // fold form
    std::vector<int> order;     // ranks, acc starts at order[0]
    uint64_t role_mask = 0;     // bit j: acc is the `out` operand at step j
    // tree form
    std::vector<TreeStep> steps;
    int result = 0;
    int nr = 0;                 // ranks referenced (inputs 0..nr-1)
    // coll/libnbc's programs: every step is the 3-buff rule op3(in1 = the `out` slot, in2 = the
    // `in` slot) (ompi_3buff_op_reduce, nbc.c:446-467) instead of op2
    bool three = false;
};

// compile an expression tree rooted at `root` over ranks [0, n)
bool compile_expr(const ExprPool &p, int root, int n, Program *out);

// ---- reference schedules, restated symbolically ----------------------------------------------
// MPI_Allreduce, recursive doubling (coll_tuned_allreduce.c:143-294): expression of the result
// (identical on every rank).
int expr_allreduce_recursive_doubling(ExprPool &p, int n);
// Ring / segmented ring (coll_tuned_allreduce.c:360-554, :635-873): element of block b ends as
// ((x_b (op) x_{b+1}) ...) with each later rank's LOCAL value as `out` and the received partial
// as `in` (:480-496).
Program ring_block_program(int n, int b);
// MPI_Reduce trees (coll_tuned_reduce.c:66-361, :618-721; topologies coll_tuned_topo.c).
// The chain (alg 2) hangs `chain_fanout` chains off the root (coll_tuned_topo.c:457-603); the
// reference's value is the MCA parameter coll_tuned_reduce_algorithm_chain_fanout (default 4,
// coll_tuned_component.c:51) or the fan-in/out of a dynamic rule.
enum ReduceAlg { RED_LINEAR = 1, RED_CHAIN = 2, RED_PIPELINE = 3, RED_BINARY = 4, RED_BINOMIAL = 5 };
constexpr int kDefaultChainFanout = 4;
int expr_reduce(ExprPool &p, int alg, int n, int root, int chain_fanout = kDefaultChainFanout);
// MPI_Reduce_scatter recursive halving (coll_tuned_reduce_scatter.c:141-400): expression of
// every rank block b (independent of rcounts).
std::vector<int> expr_reduce_scatter_rechalving(ExprPool &p, int n);
// MPI_Reduce_scatter ring (coll_tuned_reduce_scatter.c:466-636): program of block b.
Program reduce_scatter_ring_block_program(int n, int b);

// ---- decisions (coll_tuned_decision_fixed.c) --------------------------------------------------
enum AllreduceAlg { AR_DECISION = 0, AR_LINEAR = 1, AR_NONOVERLAPPING = 2, AR_RECDBL = 3, AR_RING = 4,
                    AR_RING_SEGMENTED = 5 };
int allreduce_decision(int n, size_t count, size_t dsize);            // :42-85
int reduce_decision(int n, size_t count, size_t dsize);               // :343-446 (commutative)
// reduce_scatter algorithm ids of coll/tuned (coll_tuned_reduce_scatter.c:46-52)
enum ReduceScatterAlg { RS_NONOVERLAPPING = 1, RS_RECHALVING = 2, RS_RING = 3 };
int reduce_scatter_decision(int n, size_t total_count, size_t dsize); // :456-502; RS_RECHALVING or RS_RING

// COLL_TUNED_COMPUTED_SEGCOUNT (coll_tuned.h:525-533)
size_t computed_segcount(size_t segsize, size_t typelng, size_t count);
// COLL_TUNED_COMPUTE_BLOCKCOUNT (coll_tuned.h:546-552) block offset/length
void ring_block(size_t count, int n, int b, size_t *off, size_t *len);

// ---- coll/libnbc (coll_nbc.cpp): the nonblocking reductions' own schedules -------------------
// Every reduction step of libnbc is NBC_Sched_op(target, in1, in2) = ompi_3buff_op_reduce with the
// rank's own data as in1 (nbc.c:123-145, :446-467); an op node (out, in) of these expressions is
// op3(in1 = out, in2 = in) and the compiled Program carries three = true.
enum NbcAlg { NBC_BINOMIAL = 101, NBC_RING = 102, NBC_CHAIN = 103 };
int nbc_iallreduce_decision(int n, size_t count, size_t dsize, bool inplace);  // nbc_iallreduce.c:80-85
int nbc_ireduce_decision(int n, size_t count, size_t dsize);                   // nbc_ireduce.c:74-88
// binomial tree to `root`, rank 0 and the root swapped (RANK2VRANK; nbc_ireduce.c:211-285); with
// root 0 also MPI_Iallreduce's tree (allred_sched_diss, nbc_iallreduce.c:225-272) and
// MPI_Ireduce_scatter_block's (coll_libnbc_ireduce_scatter_block.c:78-116) and MPI_Ireduce_scatter's
// (nbc_ireduce_scatter.c:84-137)
int expr_nbc_binomial(ExprPool &p, int n, int root);
int expr_nbc_reduce_chain(ExprPool &p, int n, int root);  // red_sched_chain, nbc_ireduce.c:288-340
// ring (allred_sched_ring, nbc_iallreduce.c:304-471): segment e is folded x_{e-1}, x_e, ...,
// x_{e+n-2}, every rank's own value as in1 and the received partial as in2
Program nbc_ring_segment_program(int n, int e);
// its partition (:311-329): segments of ceil(count / n), filled in order; the last non-empty one
// is short, those after it empty
void nbc_ring_block(size_t count, int n, int e, size_t *off, size_t *len);
// the program of `alg` (NbcAlg) for MPI_Iallreduce (coll 0; block = ring segment), MPI_Ireduce
// (coll 1; block = root) or MPI_Ireduce_scatter(_block) (coll 2); false: it does not fit the device
bool nbc_program(int coll, int n, int alg, int block, Program *out);

} // namespace mi355x
