// tree_extract.h — the usable subtree of a grown tree as a tree of its own, stated once for
// host and device code (no reference counterpart: the reference never prunes or re-roots).
//
// Inputs: a tree of R rows in the planner's layout (state R x 4 floats, ctrl R x 4 floats with
// the cost in .w, parent R ints), a root in [0, R) and an optional keep mask of R bytes.  With
// a null mask every row is kept; a row is kept iff its byte is non-zero (the masked query's
// rule, sbmp_goal_answer).
//
// Membership, by ascending row (a usable parent is a lower row, so one ascending loop decides):
//     row root      is a member iff it is kept; its parent word is never read, so a D6 row or a
//                   crafted orphan is a valid root
//     row r > root  is a member iff it is kept, recheck_parent_usable(parent[r], r) holds and
//                   parent[r] is a member
//     row r < root  is never a member
// Numbering: newRow[r] = the number of members below r for a member, -1 otherwise; kept = the
// number of members.  The old order is preserved: the root becomes row 0 and every new parent
// is a lower new row, so the "lowest row on ties" answers of the query commute with the
// extraction.
// Output, for each member r with k = newRow[r]: state[k] and ctrl[k] are the stored 16 bytes
// each, bit for bit (costs stay measured from the original root: the summary's rootCost is the
// stored ctrl[root].w); origin[k] = r; parent[k] = -1 for the root, else newRow[parent[r]].
// Summary: a row's class is its first match of below (r < root), masked (its byte is 0),
// detached (kept, but no member parent), kept.  A root that is not kept gives kept = 0.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sbmp/sbmp.h"
#include "sbmp/tree_recheck.h"

namespace sbmp {

SBMP_HD bool extract_row_kept(const uint8_t* keep, int r) { return !keep || keep[r] != 0; }

// The first (anc, dead) pair of the device's pointer jumping, k_tree_alive's input convention
// with another initial condition.  dead: the row cannot be a member whatever its chain holds.
// `parent` is read only where extract_reads_parent says so.
SBMP_HD bool extract_reads_parent(int r, int root, bool kept) { return r > root && kept; }
SBMP_HD bool extract_mark_dead(int r, int root, bool kept, int parent) {
    return r < root || !kept || (r > root && !recheck_parent_usable(parent, r));
}
// A dead row, the root and the rows below it point at themselves: nothing is ever loaded
// through an unusable parent word.
SBMP_HD int extract_mark_anc(int r, int root, bool dead, int parent) { return (dead || r <= root) ? r : parent; }

// A row's class, the first match (member: the row's membership as decided).
enum { kExtractKept = 0, kExtractBelow = 1, kExtractMasked = 2, kExtractDetached = 3 };
SBMP_HD int extract_row_class(int r, int root, bool kept, bool member) {
    return r < root ? kExtractBelow : !kept ? kExtractMasked : !member ? kExtractDetached : kExtractKept;
}

// The parent of new row newRow[r] (r a member).
SBMP_HD int extract_new_parent(int r, int root, const int* parent, const int* newRow) {
    return r == root ? -1 : newRow[parent[r]];
}

// Membership, numbering and the summary over host rows in one ascending loop.  newRow: rows
// ints.  0 <= root < rows.
static inline void extract_number_host(const float* ctrl, const int* parent, int rows, int root, const uint8_t* keep,
                                       int* newRow, sbmp_tree_extract* out) {
    sbmp_tree_extract s = {rows, 0, 0, 0, 0, root, ctrl[4 * (size_t)root + 3]};
    for (int r = 0; r < rows; ++r) {
        const bool kept = extract_row_kept(keep, r);
        bool member = r == root && kept;
        if (extract_reads_parent(r, root, kept)) {
            const int p = parent[r];
            member = recheck_parent_usable(p, r) && newRow[p] >= 0;
        }
        newRow[r] = member ? s.kept : -1;
        switch (extract_row_class(r, root, kept, member)) {
            case kExtractBelow: ++s.below; break;
            case kExtractMasked: ++s.masked; break;
            case kExtractDetached: ++s.detached; break;
            default: ++s.kept; break;
        }
    }
    *out = s;
}

// The members' rows into the outputs that are non-null (each of at least `kept` rows).
static inline void extract_gather_host(const float* state, const float* ctrl, const int* parent, int rows, int root,
                                       const int* newRow, float* oState, float* oCtrl, int* oParent, int* oOrigin) {
    for (int r = 0; r < rows; ++r) {
        const int k = newRow[r];
        if (k < 0) continue;
        if (oState) memcpy(oState + 4 * (size_t)k, state + 4 * (size_t)r, 16);   // bytes: a NaN keeps its pattern
        if (oCtrl) memcpy(oCtrl + 4 * (size_t)k, ctrl + 4 * (size_t)r, 16);
        if (oOrigin) oOrigin[k] = r;
        if (oParent) oParent[k] = extract_new_parent(r, root, parent, newRow);
    }
}

// The literal rule in plain loops: newRow (rows ints, required), then the outputs that are
// non-null.  The caller has checked that they hold the members (extract_number_host tells).
static inline void extract_rows_host(const float* state, const float* ctrl, const int* parent, int rows, int root,
                                     const uint8_t* keep, int* newRow, float* oState, float* oCtrl, int* oParent,
                                     int* oOrigin, sbmp_tree_extract* out) {
    extract_number_host(ctrl, parent, rows, root, keep, newRow, out);
    extract_gather_host(state, ctrl, parent, rows, root, newRow, oState, oCtrl, oParent, oOrigin);
}

}  // namespace sbmp
