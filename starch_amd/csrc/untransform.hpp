// starch_amd/csrc/untransform.hpp -- host interface of the inverse transform
// (segment texts -> BED lines).
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

struct TransformWorkspace;

namespace ut {

class Untransform {
public:
    struct Seg {
        uint64_t text_off, text_len;   // the segment's transformed text in d_text
        std::string name;              // its chromosome
    };
    // Which lines to keep (indexed extraction): segment s keeps every line
    // when whole[s], else the lines with start < qe[k] && stop > qs[k] for
    // some k in [q_lo[s], q_hi[s]).  Each segment's ranges are disjoint with
    // qs and qe increasing (touching ranges stay separate).
    struct Selection {
        std::vector<int64_t> qs, qe;
        std::vector<uint32_t> q_lo, q_hi, whole;    // one per segment
        uint64_t lines_scanned = 0, lines_out = 0;   // out: value lines seen / kept
    };
    // Merge of sorted runs (starchcat): segment s is a run of group group[s].
    // A group's segments are adjacent, in run order, and the groups appear in
    // output order (group is non-decreasing), all with the same name within a
    // group.  The output holds, group after group, the group's lines ordered
    // by (start, stop) as signed 64-bit integers; equal keys stay in run order
    // and, within a run, in their original order.  Every run of a group with
    // two or more runs must be non-decreasing in (start, stop): if one is not,
    // run() writes nothing, returns 0 and reports in bad_seg / bad_line the
    // lowest offending segment and the ordinal (from 0, counting its BED
    // lines) of its first line that sorts before its predecessor.
    struct Merge {
        static constexpr uint32_t kNone = 0xFFFFFFFFu;
        std::vector<uint32_t> group;                 // one per segment
        uint64_t lines_out = 0;                      // out: BED lines written
        uint32_t bad_seg = kNone, bad_line = 0;      // out
    };
    // BED lines of every segment, in order, into `out`; returns their bytes.
    // Throws StarchError(-12) on text the forward transform cannot have made.
    // sel == nullptr: every line.  mg != nullptr (sel must be null): the
    // groups' lines merged as described at Merge.
    uint64_t run(TransformWorkspace& tf, const uint8_t* d_text, uint64_t n, const std::vector<Seg>& segs,
                 hipStream_t st, DevBuf& out, Selection* sel = nullptr, Merge* mg = nullptr);

private:
    DevBuf b_seg, b_names, b_segfirst, b_rec, b_key, b_cd, b_contrib, b_excl, b_stop, b_olen, b_tmp, b_sel;
    DevBuf b_mkey, b_mtab, b_mrank, b_mlen;          // merge: dense keys, run table, ranks, ranked lengths
};

}  // namespace ut
