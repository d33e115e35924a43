/*
 * murbmst.h — the Euclidean minimum spanning tree of a murbhip context's bodies, and the sweep it is built from: per listed body
 * the nearest body OF ANOTHER LABEL.  What the read-outs beside it cannot answer is the structure of the system: the mass
 * segregation ratio (Allison et al. 2009: the tree length of the most massive bodies against that of random sets), the
 * normalised mean edge length (Cartwright & Whitworth 2004), and the friends-of-friends groups at EVERY linking length from one
 * tree (cut the edges longer than b and the components are the groups at b).  Boruvka's algorithm needs, per round, every
 * body's nearest body of another component: the nearest-neighbour sweep with a label compared per pair, at most ceil(log2 n)
 * times.  An interface of its own beside murbnbr.h (same library, libmurbhip.so; same conventions and return codes): the calls
 * here are read-outs in the sense of murbhip.h's call-order contract, and nothing declared in the other headers changes its
 * behaviour because of them.
 *
 * Definition (normative).  The r2 of bodies i and j is the sweeps' own fp32 value, with d = q_j - q_i:
 *       r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))
 *   r2(i, j) == r2(j, i) bit for bit (murbnbr.h), and the sweeps order candidates by (r2, index): together they make the tree
 *   below unique, so that it can be compared as an exact edge set.
 *
 * 1. murbforeign_of(ctx, count, bodies, label, partner, r2): the nearest body of another label.
 *   label holds n ints, one per body.  A value >= 0 is a group.  A value < 0 puts the body outside: it is never a candidate,
 *   and as a point it gets partner = -1, r2 = +inf.
 *   The points are the listed bodies; bodies NULL: all n bodies in order (count must then be n).  The same body may be listed
 *   twice.  For point i the result is the minimum under (r2, index j) over all real bodies j with
 *       label[j] >= 0 && label[j] != label[i]
 *   If there is no such body, or only bodies at r2 = +inf or NaN, the result is -1, +inf.  The body itself drops out by its own
 *   label: there is no skip entry.  Massless bodies are candidates; the padding slots that fill the layout never are.
 *   The bits depend on the bodies, the point and the labels alone: not on "field_chunks", "field_batch", `count`, a point's
 *   place in the list or the other points.  No atomic operation takes part.  With label[i] = i the result is murbknn_of's
 *   column 0 (k = 1) bit for bit.
 *   How a slot is made to lose.  The sweep reads a copy of the position records in which each body's label travels as bits in
 *   the place of its G m, and in which every slot that must never win (label < 0, padding) carries x = +inf.  Its r2 is then
 *   +inf for every point, which is never strictly below the running minimum (that starts at +inf).  +inf rather than NaN: the
 *   value stays an ordered number and may be compared for equality.  A slot of the point's own label is replaced by +inf
 *   through an integer compare and a select.  Labels never meet a float operation.
 *
 * 2. murbmst_of(ctx, member, capacity, ei, ej, er2, elen, label, out8): the minimum spanning forest of the bodies in the byte
 *   mask `member` (n bytes, non-zero = inside; NULL: all bodies).
 *   The order on unordered pairs is the key (r2, min(i, j), max(i, j)); the forest is Kruskal's under that key, and unique.
 *   Edges come back with ei < ej, ascending by the key; er2 is the sweep's r2 of the pair.  elen is the fp64 length from the
 *   fp32 coordinates on the device, one operation a line, none contracted:
 *       dx = (double)qx[j] - (double)qx[i]      (dy, dz likewise)
 *       len = sqrt((dx dx + dy dy) + dz dz)
 *   (the softening does not enter the length).  label holds n entries: the smallest member index of the body's component, or
 *   -1 outside the mask.  out8: {members, edges, components, rounds, total length (added in edge order), mean length (NaN
 *   without an edge), longest length, 0}.  Components exceed 1 only where pairs have r2 = +inf (the fp32 r2 overflowed).
 *   rounds counts the Boruvka rounds that added an edge: at most ceil(log2 members).
 *   Capacity.  Any of ei, ej, er2, elen, label may be NULL.  `capacity` is the number of entries each given edge array holds.
 *   If it is below the edge count, out8 and label are complete, the edge arrays are untouched, and the call returns
 *   MURBHIP_E_INVALID: the caller sizes its arrays from out8[1] (members - 1 always serves) and calls again.
 *   Its bits depend on the bodies and the mask alone.
 *   How it runs.  The points of every round are the members alone, not all n: a tree over the 50 most massive of 200 000
 *   bodies costs 50 points per round.  Per round the host uploads n labels, launches the label and pack kernels and the sweep,
 *   reads (partner, r2) of the members and runs murbmst_round.  The rounds end when one component is left or a round adds no
 *   edge.  A guard of 40 rounds returns MURBHIP_E_STATE; it is never reached, since every round at least halves the components.
 *
 * The bodies are the context's current ones on the device: positions as the last upload, initialisation or step left them.
 *   Velocities and masses are not read.  Nothing of the context changes: the calls write buffers of their own and the field
 *   read-out's point buffer, which no other call reads, and never the sweeps' partial rows, the accelerations, the remembered
 *   (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 * Call orders (murbhip.h, C1-C3).  Both are synchronous observers: deleting them from a sequence of calls changes no bit of
 *   anything read afterwards, the other read-outs included, and each returns the bits it returns as the only observer at that
 *   point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  murbforeign_of with count == 0 returns 0
 *   and does nothing, in every state.  MURBHIP_E_INVALID: a NULL context; NULL label, partner or r2 (murbforeign_of); NULL out8
 *   (murbmst_of); a body index outside [0, n); bodies NULL with count != n; an edge count beyond the capacity (above).
 * Options.  The calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field read-out's planning, and
 *   have none of their own.  With murbhip's "profile" 2 the sweep launches are recorded as spans of a kind of their own
 *   ("span_mst_ms_avg", "span_mst_count"); the force_* figures count force launches alone.
 *
 * Two host-only aids that need no device and no context:
 * murbmst_round(n, label, partner, r2, ei, ej, er2, capacity, edges): one Boruvka round.  label (n entries, read and written):
 *   >= 0 a component, < 0 outside.  partner, r2 (n entries): what murbforeign_of returns for these labels and all bodies; read
 *   at the bodies with label >= 0 alone; partner -1: none.  Per component the call takes the minimum, by the key, over its
 *   bodies' (i, partner[i], r2[i]); the union of the chosen edges, the edge two components choose mutually taken once, is
 *   appended in key order to the edge arrays behind the *edges entries they hold (any array may be NULL), *edges grows by the
 *   number added, and every body of a merged component is relabelled to the component's smallest body index.  An edge that
 *   would close a cycle, or a partner outside [0, n), outside the labelled bodies or of the body's own label, means the input
 *   is not what murbforeign_of returns for these labels: MURBHIP_E_INVALID, and nothing is changed.  Likewise when the edges
 *   would not fit `capacity`, and for NULL label, partner, r2 or edges.
 * murbmst_cut(n, edges, ei, ej, er2, thr, label): single-linkage groups, the components under the edges with r2 <= thr.  The
 *   label is the component's smallest body index; bodies on no edge label themselves.  With thr = murbnbr_threshold(b, soft)
 *   and the tree of all bodies this equals friends-of-friends at linking length b: the pairs with r2 <= thr are a down-set of
 *   the key's order, so Kruskal's forest restricted to them is a spanning forest of that graph.  MURBHIP_E_INVALID: an edge
 *   index outside [0, n), a NaN thr, a NULL array that is needed.
 *
 * Not covered: Cartwright & Whitworth's Q (its mean pair separation is an fp32 N^2 sum of another kind); several shards or
 *   ranks; block-open states; arbitrary points (the points are bodies: a point needs a label); a tree kept on the device; the
 *   murb-hip command line.
 */
#ifndef MURBMST_H_
#define MURBMST_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbforeign_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const int* label, int* partner, float* r2);
int murbmst_of(murbhip_ctx* ctx, const unsigned char* member, unsigned long capacity, int* ei, int* ej, float* er2, double* elen,
               int* label, double* out8);

int murbmst_round(unsigned long n, int* label, const int* partner, const float* r2, int* ei, int* ej, float* er2,
                  unsigned long capacity, unsigned long* edges);
int murbmst_cut(unsigned long n, unsigned long edges, const int* ei, const int* ej, const float* er2, float thr, int* label);

#ifdef __cplusplus
}
#endif

#endif
