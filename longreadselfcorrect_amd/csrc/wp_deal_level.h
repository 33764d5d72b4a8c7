// wp_deal_level.h -- the levels of LRSC_WP_DEAL (WpArgs::deal_level, wp_deal_step.h's deal_step): how much of a lane-per-walk
// wavefront's general step is dealt across its lanes.  One place for the default, which read_tunables (capi_core.cpp) and the
// host harnesses (tests/host_walk_deal*, which call deal_step without a level) both take.
#pragma once
#include <cstdint>

namespace lrsc {

constexpr uint32_t kDealLevelExtend = 1;     // extendLeaves: refineSAInterval, attempToExtend (deal_refine, deal_attempt)
constexpr uint32_t kDealLevelPrune = 2;      // + PrunedBySeedSupport (deal_prune)
constexpr uint32_t kDealLevelTerm = 3;       // + isTerminated's scans over the new frontier (deal_term)
constexpr uint32_t kDealLevelDefault = kDealLevelExtend;    // neither later phase won its A/B ("The prune and isTerminated dealt")

} // namespace lrsc
