// stream_set_plan_driver -- runs speechrecognition_amd/csrc/stream_set_plan.h (host code, no HIP) for tests/test_stream_set_cpu.py.
// Input file, a command per line, an answer line per command:
//   set <max_streams> <max_frames>              a fresh set of slots                         -> set
//   begin                                       StreamSlots::begin                           -> begin <slot> <id>   |  begin -1
//   end <slot>                                  what an _end call does to the slot           -> end
//   gen <slot> <generation>                     sets the slot's next generation              -> gen
//   find <id>                                   StreamSlots::find                            -> find <slot or -1>
//   resolve <n> <id> ...                        resolve_ids                                  -> resolve <entry> <fault> <slot> ... (entry of them)
//   resolve24 <n> <id> ...                      ... into the first field of 24-byte records  -> likewise
//   window <max_frames> <base> <have> <add>     check_window                                 -> window <fault>
//   layout <job> <result> <frame> <n> <F>       block_layout (sizes in bytes)                -> layout <res_at> <items_at> <need>
//   grown <need> <have>                         block_grown                                  -> grown <bytes>
// resolve's slots are an allocation of exactly n entries (records): a write past the entries named is a write past it.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "stream_set_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s commands.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  srplan::StreamSlots sl;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    unsigned long long a = 0, b = 0, c = 0, d = 0, e = 0;
    if (cmd == "set") {
      ls >> a >> b;
      sl = srplan::StreamSlots((uint32_t)a, b);
      printf("set\n");
    } else if (cmd == "begin") {
      const int64_t slot = sl.begin();
      if (slot < 0) printf("begin -1\n");
      else printf("begin %lld %u\n", (long long)slot, sl.id.at(slot));
    } else if (cmd == "end") {
      ls >> a;
      sl.open.at(a) = 0;
      printf("end\n");
    } else if (cmd == "gen") {
      ls >> a >> b;
      sl.generation.at(a) = (uint32_t)b;
      printf("gen\n");
    } else if (cmd == "find") {
      ls >> a;
      printf("find %lld\n", (long long)sl.find((uint32_t)a));
    } else if (cmd == "resolve") {
      ls >> a;
      std::vector<uint32_t> ids(a), slots(a, 0xFFFFFFFFu);
      for (auto& i : ids) { ls >> b; i = (uint32_t)b; }
      const srplan::IdResolution r = srplan::resolve_ids(sl, (uint32_t)a, ids.data(), slots.data());
      printf("resolve %u %d", r.entry, (int)r.fault);
      for (uint32_t i = 0; i < r.entry; i++) printf(" %u", slots.at(i));
      printf("\n");
    } else if (cmd == "resolve24") {
      struct Record { uint32_t slot, rest[5]; };
      static_assert(sizeof(Record) == 24, "a StableJob's size");
      ls >> a;
      std::vector<uint32_t> ids(a);
      std::vector<Record> recs(a, Record{0xFFFFFFFFu, {1, 2, 3, 4, 5}});
      for (auto& i : ids) { ls >> b; i = (uint32_t)b; }
      const srplan::IdResolution r = srplan::resolve_ids(sl, (uint32_t)a, ids.data(), a ? &recs[0].slot : nullptr, sizeof(Record));
      printf("resolve %u %d", r.entry, (int)r.fault);
      for (uint32_t i = 0; i < r.entry; i++) printf(" %u", recs.at(i).slot);
      for (const Record& x : recs)
        if (x.rest[0] != 1 || x.rest[4] != 5) { fprintf(stderr, "a record's other fields were written\n"); return 3; }
      printf("\n");
    } else if (cmd == "window") {
      ls >> a >> b >> c >> d;
      printf("window %d\n", (int)srplan::check_window(a, b, c, d));
    } else if (cmd == "layout") {
      ls >> a >> b >> c >> d >> e;
      const srplan::BlockLayout at = srplan::block_layout(a, b, c, (uint32_t)d, e);
      printf("layout %zu %zu %zu\n", at.res_at, at.items_at, at.need);
    } else if (cmd == "grown") {
      ls >> a >> b;
      printf("grown %zu\n", srplan::block_grown(a, b));
    } else {
      fprintf(stderr, "bad command: %s\n", line.c_str());
      return 2;
    }
    if (!ls) { fprintf(stderr, "bad command: %s\n", line.c_str()); return 2; }
  }
  return 0;
}
