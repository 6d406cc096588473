// resolve_rounds.hip.h -- the rounds of the two claim resolvers, k_proj_resolve (projection_search.hip.h) and k_init_resolve
// (init_search.hip.h): one workgroup per problem turns a loop the reference runs sequentially over the queries into rounds.
//
// Why rounds end at the sequential answer.  In both searches what query q may take depends on what the queries < q took: the claim rule of
// SearchByProjection (a keypoint an earlier query claimed is skipped), the retraction rule of SearchForInitialization (a keypoint an earlier
// query accepted at a smaller or equal distance is skipped).  It is a triangular system -- query q depends on queries < q only.  Every round
// rebuilds the claim state from the matches of the previous round and re-evaluates all queries against it, until a round changes no match;
// the only fixed point of that iteration is the sequential answer (induction over q), and when the smallest query a round changed is c, every
// query <= c is final -- queries < c were evaluated against a final prefix and did not move, and c itself was evaluated against that same
// prefix -- so the next round starts at c + 1: at most nq rounds, whatever the data.
//
// A round: rebuild the claim state from the matches; one THREAD per query >= lo settles it from its K-list or lists it for a re-search; the WAVES
// then search the listed queries below the cut again in full.  The kernels keep their loop bodies -- one loop taking the steps as callables made
// a resolver 0.2-0.6 % slower (profiles/search_refactor.md) -- and share what decides termination: the cut and the advance of lo.
//
// Cost of the worst case.  The lists and the round loop are sized for the usual scene, where a handful of rounds settle everything and
// few lists run out.  When many queries sit on one spot, every round settles one query (lo advances by one) and every later query's
// list is exhausted.  Searching all of those again each round would be about nq^2 / 2 full walks on one CU, every one of them stale
// but the first; so a round walks only the queries below a cut T = lo + max(16, (nq - lo) * XFH_RESOLVE_REDO_BUDGET / nredo), which holds
// about XFH_RESOLVE_REDO_BUDGET of them when they are spread evenly, and postpones the rest: their match stays as it was, the smallest
// postponed query bounds the next round's lo from above, and the loop does not end while one is postponed (lo itself is always below
// the cut, so every round still settles at least one query).  The worst case is then nq rounds of at most max(16, BUDGET) walks of up
// to nt candidates each -- nq = nt = XFH_GRID_MAX_N on one spot is about 10^6 walks of 16384 distances on ONE CU, i.e. seconds, not
// milliseconds: exact and terminating, as the contract asks, and nothing more.  A caller with such input should not expect frame rate.
#pragma once
#include "ctx.h"

#define XFH_RESOLVE_REDO_BUDGET 64                                     // full walks a round aims at (four per wave of a 1024-thread workgroup)
#define XFH_RESOLVE_NONE 0x7fffffff                                    // no query: larger than every query number

// The two formulas are macros, not functions: as inlined functions they compiled to other scalar code for the cut, and the resolvers' machine code
// is to stay what it was (profiles/search_refactor.md).
// the first query a round does NOT search again in full when nredo lists ran out ("Cost of the worst case")
#define XFH_RESOLVE_CUT(lo, nq, nredo) ((nredo) <= XFH_RESOLVE_REDO_BUDGET ? (nq) : (lo) + max(16, (int)((long long)((nq) - (lo)) * XFH_RESOLVE_REDO_BUDGET / (nredo))))
// the next round's first query; c: the smallest query the round moved, d: the smallest it postponed (XFH_RESOLVE_NONE: none; the loop ends when both
// are).  Queries < min(c, d) were evaluated against a final prefix and did not move
#define XFH_RESOLVE_NEXT_LO(c, d) ((c) == XFH_RESOLVE_NONE ? (d) : min((c) + 1, (d)))
