// het_grouping: positions of an index list sorted by (relation, key), with the
// segments (runs of equal (relation, key)) and a list of wave-sized work items.
#pragma once
#include <vector>

#include "common.hip.h"

// Segments longer than this are split into several work items so that no single
// wave serialises a hub node (degree skew: a few destinations own 1e5+ edges).
constexpr int HET_ITEM_MAX = 256;

struct het_grouping {
  uint64_t serial = 0;     // unique per object for the life of the process (an address can come back after a destroy)
  // Ownership.  Every device array below, built by het_grouping_create or on first use, comes from grouping_alloc: allocated on
  // `home`, the stream the grouping was created on (with a stream-ordered allocator -- het_set_allocator -- the block belongs to
  // that stream's pool), on `device`, and listed in `blocks` until het_grouping_destroy.  `used`: the other streams that read the
  // arrays (het_grouping_note_stream, and every stream a list was built on); destroy makes `home` wait for them before it
  // releases anything.  A list that a rebuild replaces is only un-published: its block stays in `blocks` (a launch of another
  // thread may still read it).
  struct Block { void* ptr; size_t bytes; };
  hipStream_t home = nullptr;
  int device = 0;
  mutable std::vector<hipStream_t> used;
  mutable std::vector<Block> blocks;
  int64_t E = 0;           // positions
  int64_t S = 0;           // segments
  int64_t num_items = 0;   // work items (>= S)
  int64_t num_split = 0;   // segments that were split into > 1 item
  int64_t key_bound = 0;
  int R = 0;               // 0: grouped by key only
  int32_t* perm = nullptr;       // [E]   position at sorted rank j (stable)
  int32_t* seg_ptr = nullptr;    // [S+1] sorted-rank range of segment s
  int32_t* seg_key = nullptr;    // [S]   key of segment s
  int32_t* seg_rel_ptr = nullptr;// [R+1] segment range of relation r (R > 0)
  idx_t* seg_key64 = nullptr;    // [S]   seg_key as int64 (gather / scatter list of the segment GEMMs)
  idx_t* seg_rel_ptr64 = nullptr;// [R+1] seg_rel_ptr as int64
  int32_t* item_seg = nullptr;   // [num_items] segment of the item
  int32_t* item_begin = nullptr; // [num_items+1] sorted-rank range [item_begin[t], item_end[t])
  int32_t* item_end = nullptr;
  int32_t* split_seg = nullptr;  // [num_split] segments that own several items
  int32_t* p0 = nullptr;         // [E] payload0[perm[j]] or NULL
  int32_t* p1 = nullptr;         // [E] payload1[perm[j]] or NULL
  int64_t p0_max = 0, p1_max = 0;  // largest payload value (0 without the payload): bounds the tables a kernel indexes with them
  bool p0_contiguous = false;    // p0[j] == j for every rank: the list already was in (relation, key) order
  mutable int32_t* seg_of_rank = nullptr;  // [E] segment of sorted rank j; built on first use (segment broadcast)
  // "Packs" (grouping_packs): the SHORT segments (<= HET_PACK_T positions) gathered into runs of whole segments of about
  // HET_PACK_T consecutive ranks (< 2 * HET_PACK_T) -- the work unit of the lane-group-per-pack kernels; a few edges per
  // (relation, source) row is the common case, and a work unit per segment would spend its time in dependent
  // prologues.  A longer segment is a pack of its own with bit 31 of pack_ptr set: the pack kernels skip it and the
  // wave-per-item kernels take its work items (long_items: indices into item_seg / item_begin / item_end).
  mutable int32_t* pack_ptr = nullptr;     // [num_packs+1] first rank of pack k (| 1u<<31: a long segment)
  mutable int32_t* key_of_rank = nullptr;  // [E+1] seg_key of the segment of rank j; sentinel -1 at E
  mutable int32_t* long_items = nullptr;   // [num_long_items] work items of segments with more than HET_PACK_T positions
  mutable int64_t num_packs = 0, num_long_items = 0;
  // A second set of packs for ONE other threshold (grouping_pack_view: the RGAT backward walks segments of up to 64 positions in
  // packs), kept beside the default set, so that the packs an op gets do not depend on which op touched the grouping first
  // (until round 5 the first user's threshold decided for everybody, and with it the fp32 summation order).
  mutable int32_t* alt_pack_ptr = nullptr;
  mutable int32_t* alt_long_items = nullptr;
  mutable int64_t alt_num_packs = 0, alt_num_long_items = 0;
  mutable int alt_pack_t = 0;              // 0: not built
  // Packed ids (grouping_packed_ids): one vector load per edge instead of one per list -- the gather passes are bound by the
  // number of their vector-memory instructions.
  mutable int2* p01 = nullptr;    // [E]   {p0[j], p1[j]}
  mutable int4* kp01 = nullptr;   // [E+1] {key_of_rank[j], p0[j], p1[j], tag}; sentinel key -1 at E (needs the packs)
  // tag (grouping_tag_kp01; 0 until a user asks): what a lane group that walks the ranks of a pack in order would otherwise derive
  // from compares against the neighbouring records and a search of relation boundaries, per edge --
  //   HET_TAG_FIRST_KEY / _LAST_KEY  first / last rank of its segment;  HET_TAG_LAST_RUN  last rank of a run of equal p1 inside it
  //   tag >> HET_TAG_REL_SHIFT  relation of the rank: number of relation boundaries <= its key (tag_which 0) or its p0 (tag_which 1)
  mutable int tag_which = -1;     // -1: not tagged
  mutable int tag_thr[7] = {0, 0, 0, 0, 0, 0, 0};
  mutable const idx_t* tag_dev_src = nullptr;  // grouping_tag_kp01_dev: the device array the boundaries were read from (the caller pins it), its length - 1
  mutable int tag_dev_R = 0;
  // Hub items (grouping_hub_items): for a grouping by key * R + relation, the work items (ascending) whose key belongs to a
  // segment of more than hub_min positions in the twin grouping by key alone (het_rgat_aggregate_compact_runs).
  mutable int32_t* hub_items = nullptr;
  mutable int64_t num_hub_items = -1;         // -1: not built
  mutable int32_t* hub_order = nullptr;       // [num_hub_items] indices into hub_items, by the first payload0 of the twin in the item
  mutable int32_t* hub_segs = nullptr;        // the twin's segments of more than hub_min positions (ascending)
  mutable int4* hub_rec = nullptr;            // [num_hub_segs] {first run (segment of this grouping), one past the last, first record in
                                              // hub_items, key of the hub}: what a finishing pass needs per hub, searched ONCE here
                                              // instead of by five dependent binary searches per hub and launch (round 5)
  mutable int64_t num_hub_segs = 0;
  mutable int hub_min = 0;
  mutable uint64_t hub_twin_serial = 0;       // serial of the twin the lists were built against
  // An order of the rows of a caller's list by the list's values (grouping_value_order).
  mutable int32_t* val_order = nullptr;
  mutable const idx_t* val_order_src = nullptr;  // key: identity only -- the order is a locality hint, any permutation of [0, n) gives the same results
  mutable int64_t val_order_n = 0;
};

// What a kernel takes of a grouping, by value: its work items, and its packs.  Kernel parameter types, so they live in an
// anonymous namespace like the kernels of the files that use them (a type at global scope would change their mangled names).
namespace {
struct Items {
  const int32_t *seg, *begin, *end, *seg_ptr, *seg_key;
  int64_t n;
};
struct Packs {
  const int32_t *ptr, *key;
  int64_t n;
};
inline Items items_of(const het_grouping* g) {
  return Items{g->item_seg, g->item_begin, g->item_end, g->seg_ptr, g->seg_key, g->num_items};
}
}  // namespace

// ---- arrays built on first use ----------------------------------------------------------------------------------------------
// One protocol for all of them (GroupingBuild, grouping.hip), one lock, and the ownership rule above:
//     GroupingBuild b(g, s);                        // takes the lock
//     if (<the slot's key is the one asked for>) return HET_OK;  // steady state: the lock and a few compares
//     <un-publish what the slot held>;              // (its blocks stay with the grouping)
//     b.begin();                                    // g's device current; `s` ordered after `home`, noted as a user
//     grouping_alloc(g, &p, bytes); launches on s;  // any early return releases what was allocated since begin()
//     if (int rc = b.finish()) return rc;           // hipStreamSynchronize(s): users may be on other streams
//     <publish pointers, counts and key>;
// A list that needs another one builds that one BEFORE its own begin() (the lock is recursive; packs need seg_of_rank, kp01
// needs the packs, tags need kp01).
int grouping_alloc(const het_grouping* g, void** out, size_t bytes);  // on g->home, recorded in g->blocks
struct OnDevice {  // makes a device current until the end of a scope
  int prev = -1;
  void enter(int dev) {
    if (hipGetDevice(&prev) != hipSuccess || prev == dev || hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
  }
  ~OnDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct GroupingBuild {
  GroupingBuild(const het_grouping* g, hipStream_t s);
  ~GroupingBuild();
  // wait_for_users: `s` also waits for every noted stream (a rebuild IN PLACE: launches there may still read the old contents)
  void begin(bool wait_for_users = false);
  int finish();
  GroupingBuild(const GroupingBuild&) = delete;
  GroupingBuild& operator=(const GroupingBuild&) = delete;

 private:
  const het_grouping* g;
  hipStream_t s;
  OnDevice device;
  size_t mark = 0;       // g->blocks.size() at begin()
  bool open = false;
};

constexpr int HET_PACK_T = 32;
// g->pack_ptr / key_of_rank / long_items for the threshold HET_PACK_T.  Key: pack_ptr set.
int grouping_packs(const het_grouping* g, hipStream_t s);
// The packs of a grouping for a threshold: HET_PACK_T (or <= 0) = the default set above; any other value = the second set
// (key: alt_pack_t; a grouping keeps one other threshold -- asking for a third replaces the second).  key_of_rank is shared.
struct PackView {
  const int32_t* pack_ptr = nullptr;
  const int32_t* long_items = nullptr;
  int64_t num_packs = 0, num_long_items = 0;
};
int grouping_pack_view(const het_grouping* g, hipStream_t s, int pack_t, PackView* out);
// g->p01 (with_keys == false) or g->kp01 (true; builds the packs first).  Key: the pointer set.
int grouping_packed_ids(const het_grouping* g, bool with_keys, hipStream_t s);
constexpr int HET_TAG_FIRST_KEY = 1, HET_TAG_LAST_RUN = 2, HET_TAG_LAST_KEY = 4, HET_TAG_REL_SHIFT = 8;
// Fills the fourth word of g->kp01 (builds kp01 first).  thr[0..6]: ascending first values of relations 1 .. 7 (INT_MAX beyond the
// last relation), or NULL: the caller reads the segment / run flags only (any tagging will do); which = 0: the relation follows the
// key, 1: payload0.  Key: (which, thr).  Another key re-tags IN PLACE (the flags are rewritten with the same values), ordered
// after every stream that uses the grouping.
int grouping_tag_kp01(const het_grouping* g, int which, const int* thr, hipStream_t s);
// The same with the relation boundaries read on the device: rel_ptrs_dev [R+1] (int64), any R < 2^23 (a search above 8).  No host
// copy (a synchronisation per call), so the key is the identity (which, array, R): the caller keeps the array alive and unchanged
// while the grouping lives (het_amd/kernels.py pins it on the Grouping and refuses an in-place edit).
int grouping_tag_kp01_dev(const het_grouping* g, int which, const idx_t* rel_ptrs_dev, int R, hipStream_t s);
// g_rel->hub_items / hub_segs / hub_order / hub_rec: g_rel groups the same positions as `twin` by key * R + relation.  Key: (serial
// of the twin object, hub_min) -- a cache that evicted and rebuilt the grouping by key alone gets new lists.
int grouping_hub_items(const het_grouping* g_rel, const het_grouping* twin, int R, int hub_min, hipStream_t s);
// g->val_order [n]: the indices of values[0..n) (device, 0 <= values < 2^31) in ascending order of the value, ties in index order.
// Key: (array, n).  A pass over the rows of a (relation, node) list in this order visits the rows of one node together
// (het_rgat_backward_compact_runs: the two rows of a destination read the same gradout / ret rows).
int grouping_value_order(const het_grouping* g, const idx_t* values, int64_t n, hipStream_t s);
