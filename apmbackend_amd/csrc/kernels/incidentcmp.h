// K25: one step of the ic stream's state machine (docs/INCIDENTS.md), shared by the kernel of
// incident.hip and the host (bindings.cpp incident_step).  One state per (series, source), one
// step per rollover, integers only:
//
//   1. hot:   hot_run = min(hot_run + 1, 255), clear_run = 0
//      clear: clear_run = min(clear_run + 1, 255), hot_run = 0
//   2. closed (code0 == 0), hot and hot_run >= open_after: code0 = code, since_ts = edge_ts,
//      age = 0, event O
//   3. open (before this step): age = min(age + 1, 2^32 - 1), then exactly one of
//        clear and clear_run >= close_after:        event C, code0 = 0 (the caller prints the row
//                                                   from the returned `code0` first: see IncidentOut)
//        remind_every != 0 and age % remind_every == 0: event S
//      a hot series whose code differs from code0 stays in the same incident.
//
// Bounds: open_after, close_after 1 .. 255 -- the runs saturate at 255, so a threshold of 255 is
// still reached; remind_every 0 .. 65535; code a printable letter when hot (ignored otherwise).
// Nothing here can overflow: the runs are compared before they are incremented, age likewise.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace apm {

struct IncidentState {  // 16 bytes
  long long since_ts;   // edge ts of the rollover that opened the incident
  uint32_t age;         // rollovers since then (0 at the opening one), saturating
  uint8_t code0;        // the code it opened with; 0: closed
  uint8_t hot_run;      // consecutive hot rollovers, saturating at 255
  uint8_t clear_run;    // consecutive clear rollovers, saturating at 255
  uint8_t pad;
};
static_assert(sizeof(IncidentState) == 16, "IncidentState is 16 bytes");

constexpr uint8_t IC_NONE = 0, IC_OPEN = 'O', IC_STILL = 'S', IC_CLOSE = 'C';

// what the row of this step prints: the state before a close wipes code0
struct IncidentOut {
  uint8_t event;        // IC_NONE / IC_OPEN / IC_STILL / IC_CLOSE
  uint8_t code0;        // the incident's opening code (also on a C row)
  uint8_t run;          // hot_run when hot, clear_run otherwise
  uint8_t pad;
  uint32_t age;
  long long since_ts;
};

__host__ __device__ inline IncidentOut incident_step(IncidentState& st, bool hot, uint8_t code, long long edge_ts,
                                                     uint32_t open_after, uint32_t close_after, uint32_t remind_every) {
  const bool was_open = st.code0 != 0;
  if (hot) {
    if (st.hot_run < 255) ++st.hot_run;
    st.clear_run = 0;
  } else {
    if (st.clear_run < 255) ++st.clear_run;
    st.hot_run = 0;
  }
  IncidentOut o{};
  o.event = IC_NONE;
  if (!was_open) {
    if (hot && st.hot_run >= open_after) {
      st.code0 = code;
      st.since_ts = edge_ts;
      st.age = 0;
      o.event = IC_OPEN;
    }
  } else {
    if (st.age < 0xffffffffu) ++st.age;
    if (!hot && st.clear_run >= close_after) o.event = IC_CLOSE;
    else if (remind_every != 0 && st.age % remind_every == 0) o.event = IC_STILL;
  }
  o.code0 = st.code0;
  o.run = hot ? st.hot_run : st.clear_run;
  o.age = st.age;
  o.since_ts = st.since_ts;
  if (o.event == IC_CLOSE) st.code0 = 0;
  return o;
}

// hot / code of one source from its record's verdict word (kernel_api.h: BurnRec.fired,
// TrafficRec.verdict, PeerRec.verdict, ShiftRec.verdict).  0: not hot.
constexpr int IC_SB = 0, IC_TF = 1, IC_PO = 2, IC_LS = 3, IC_SOURCES = 4;
__host__ __device__ inline uint8_t incident_code(int kind, int32_t word) {
  if (kind == IC_SB) return word != 0 ? 'B' : 0;
  if (kind == IC_PO) return word == 1 ? 'H' : word == 2 ? 'L' : 0;  // PO_H / PO_L
  // tf / ls: two bits per rule, rule 0 lowest; 1 = D (tf) / U (ls), 2 = S (tf) / D (ls)
  for (int j = 0; j < 4; ++j) {
    const int v = (word >> (2 * j)) & 3;
    if (v == 1) return kind == IC_TF ? 'D' : 'U';
    if (v == 2) return kind == IC_TF ? 'S' : 'D';
  }
  return 0;
}

}  // namespace apm
