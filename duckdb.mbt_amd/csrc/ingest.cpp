// ingest.cpp — device tables: creation, growth, zone maps and code images,
// INSERT ... SELECT / CREATE TABLE AS appends and the host appender's H2D path.
#include <algorithm>
#include <chrono>
#include <thread>

#include "exec.h"
#include "hostlink.h"
#include "knobs.h"

namespace mbx {
// ---------------------------------------------------------------------------
// tables: creation, append, stats
// ---------------------------------------------------------------------------
Table::~Table() {}  // column buffers go with their owners (a live result may still hold them)

TablePtr CreateDeviceTable(Connection &c, const std::string &name, const std::vector<std::string> &names,
                           const std::vector<LogicalType> &types) {
  if (c.sharded()) {
    auto t = std::make_shared<Table>();
    t->name = name;
    t->col_names = names;
    t->device = c.engine->device;
    for (auto &ty : types) {
      DevColumn dc;
      dc.type = ty;
      dc.phys = PhysOf(ty);
      t->cols.push_back(dc);
    }
    std::string key = name;
    for (auto &ch : key) ch = (char)tolower((unsigned char)ch);
    for (auto &sc : c.shards) {
      TablePtr p = CreateDeviceTable(*sc, name, names, types);
      sc->catalog.tables[key] = p;
      t->parts.push_back(p);
    }
    return t;
  }
  auto t = std::make_shared<Table>();
  t->name = name;
  t->col_names = names;
  t->device = c.engine->device;
  for (auto &ty : types) {
    DevColumn dc;
    dc.type = ty;
    dc.phys = PhysOf(ty);
    dc.stats_valid = true;
    dc.imin = 0;
    dc.imax = 0;
    t->cols.push_back(dc);
  }
  return t;
}

void DropDeviceTable(Table &t) { (void)t; }

// a table buffer from hipMalloc, freed when its last holder lets go (the
// column, or a result reading it in place; possibly on another thread)
static std::shared_ptr<void> DevOwned(Engine &e, void *p) {
  const int dev = e.device;
  return std::shared_ptr<void>(p, [dev](void *q) {
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
    (void)hipFree(q);
    if (prev != dev && prev >= 0) (void)hipSetDevice(prev);
  });
}

static void Grow(Engine &e, DevColumn &c, int64_t nrows_old, int64_t need) {
  if (need <= c.capacity && (c.phys != P_STR || c.offsets)) return;
  int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1024, c.capacity * 2));
  if (c.phys == P_STR) {
    int64_t *no = nullptr;
    HIPCHK(hipMalloc(&no, (cap + 1) * 8));
    if (c.offsets) HIPCHK(hipMemcpyAsync(no, c.offsets, (nrows_old + 1) * 8, hipMemcpyDeviceToDevice, e.stream));
    else HIPCHK(hipMemsetAsync(no, 0, 8, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.offsets_owner = DevOwned(e, no);
    c.offsets = no;
  } else {
    void *nd = nullptr;
    int sz = PhysSize(c.phys);
    HIPCHK(hipMalloc(&nd, (size_t)cap * sz));
    if (c.data && nrows_old) HIPCHK(hipMemcpyAsync(nd, c.data, (size_t)nrows_old * sz, hipMemcpyDeviceToDevice, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.data_owner = DevOwned(e, nd);
    c.data = nd;
  }
  if (c.validity) {
    uint64_t *nv = nullptr;
    HIPCHK(hipMalloc(&nv, Words64(cap) * 8));
    HIPCHK(hipMemsetAsync(nv, 0xFF, Words64(cap) * 8, e.stream));
    HIPCHK(hipMemcpyAsync(nv, c.validity, Words64(nrows_old) * 8, hipMemcpyDeviceToDevice, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.validity_owner = DevOwned(e, nv);
    c.validity = nv;
  }
  c.capacity = cap;
}

// Brings c's code image (scan_codes.h) up to nrows rows, once the zone map of
// every row is folded: the appended tail when the map still fits the image's
// base and field width, all rows when the base or the field width changed
// (the table growing past mbx_scan_codes_bits_min_rows changes it once), and
// no image when the column does not qualify.  The word that holds the first
// appended row is rebuilt whole from the values, never read back.  A column is
// never left partly coded beyond this call: code_rows is nrows or the image
// is gone.
// A table of mbx_scan_codes_planes_min_rows rows or more keeps codes of at
// most 8 bits as bit planes (scan_planes.h) instead of fields: the same rules
// with the bits per code in place of the field count (the table crossing that
// floor, or the bits per code changing, rebuilds the image once, as the other
// kind where the codes outgrow 8 bits), and a regrown buffer takes over the
// used whole segments.
// With mbx_scan_hist a plane image comes with the histogram of its codes
// (scan_hist.h), counted by the same encode pass over the same rows: this
// function is the only writer of both, so whatever drops the image (no zone
// map, NULLs, codes past 8 bits, too few rows, the option off) drops the
// histogram (as does a table below mbx_scan_hist_min_rows rows), whatever rebuilds it (CREATE OR REPLACE or a first append, a moved
// imin, other bits per code, the table crossing the planes floor) zeroes and
// recounts it, and an extended or regrown image adds the appended rows to it.
void UpdateScanCodes(Engine &e, DevColumn &c, int64_t nrows) {
  int f = 0, pb = 0;
  if (e.scan_codes && nrows > 0 && nrows >= e.scan_codes_min_rows && c.stats_valid && !c.validity &&
      c.null_count == 0 && c.data) {
    f = ScanCodeFields(c.phys, c.imin, c.imax, nrows >= e.scan_codes_bits_min_rows);
    if (f && nrows >= e.scan_codes_planes_min_rows) pb = ScanPlaneBits(c.phys, c.imin, c.imax);
    if (pb) f = 0;
  }
  const bool hist = pb && e.scan_hist && nrows >= e.scan_hist_min_rows;
  if (!hist) {  // the histogram goes with the plane image, or with the option
    c.code_hist = nullptr;
    c.code_hist_owner.reset();
    c.DropHistMirror();
  }
  if (!f && !pb) {
    c.codes = nullptr;
    c.codes_owner.reset();
    c.code_fields = c.code_planes = 0;
    c.code_base = c.code_rows = c.code_cap = 0;
    return;
  }
  // (an image that should have a histogram and has none, built while the option
  // was off or below mbx_scan_hist_min_rows rows, is rebuilt: only a pass over
  // every row can count it)
  const bool extend = c.codes && c.code_fields == f && c.code_planes == pb && c.code_base == (int64_t)c.imin &&
                      c.code_rows <= nrows && (!hist || c.code_hist);
  const int64_t begin = extend ? c.code_rows : 0;
  if (begin == nrows) return;
  // from here on the histogram is rebuilt (zeroed and recounted), or extended
  // or regrown by the appended rows: the host mirror no longer describes it
  c.DropHistMirror();
  if (!extend || c.code_cap < nrows) {
    const int64_t cap = std::max<int64_t>(nrows, c.capacity);
    const int64_t bytes = pb ? ScanPlaneBufferBytes(pb, cap) : (ScanCodeWords(f, cap) * 4 + 255) & ~(int64_t)255;
    void *nc = nullptr;
    HIPCHK(hipMalloc(&nc, (size_t)bytes));
    if (begin > 0) {
      const int64_t used = pb ? ScanPlaneBufferBytes(pb, begin) : ScanCodeWords(f, begin) * 4;
      HIPCHK(hipMemcpyAsync(nc, c.codes, (size_t)used, hipMemcpyDeviceToDevice, e.stream));
      HIPCHK(hipStreamSynchronize(e.stream));  // before the old image goes
    }
    c.codes_owner = DevOwned(e, nc);
    c.codes = nc;
    c.code_cap = cap;
    c.code_fields = f;
    c.code_planes = pb;
    c.code_base = (int64_t)c.imin;
  }
  if (hist && !extend) {  // a rebuilt image counts every row again, into 1 << pb zeroed counters
    void *nh = nullptr;
    HIPCHK(hipMalloc(&nh, (size_t)ScanHistBytes(pb)));
    c.code_hist_owner = DevOwned(e, nh);
    c.code_hist = nh;
    HIPCHK(hipMemsetAsync(nh, 0, (size_t)ScanHistBytes(pb), e.stream));
  }
  if (pb) {
    const int64_t first = begin / 32 * 32;  // the first row of the first rebuilt word of every plane
    ProfScope ps(e, "scan_encode",
                 (double)(nrows - first) * PhysSize(c.phys) +
                     (double)(ScanPlaneScanBytes(pb, nrows) - ScanPlaneScanBytes(pb, first)),
                 nrows - first);
    dev::ScanEncodePlanes(c.data, c.phys, c.codes, pb, c.code_base, begin, nrows, c.code_hist, e.stream);
  } else {
    const int64_t first = begin / f * f;  // the first row of the first rebuilt word
    ProfScope ps(e, "scan_encode",
                 (double)(nrows - first) * PhysSize(c.phys) + (double)(ScanCodeBytes(f, nrows) - ScanCodeBytes(f, first)),
                 nrows - first);
    dev::ScanEncode(c.data, c.phys, c.codes, f, c.code_base, begin, nrows, e.stream);
  }
  c.code_rows = nrows;
}

static void EnsureValidity(Engine &e, DevColumn &c, int64_t nrows_old) {
  if (c.validity) return;
  int64_t cap = std::max<int64_t>(c.capacity, 1);
  HIPCHK(hipMalloc(&c.validity, Words64(cap) * 8));
  c.validity_owner = DevOwned(e, c.validity);
  HIPCHK(hipMemsetAsync(c.validity, 0xFF, Words64(cap) * 8, e.stream));
  (void)nrows_old;
}

// the zone map the producing kernel left on d (DCol::zn), folded in instead of
// a statistics pass over the appended rows
static bool FoldKernelStats(DevColumn &c, const DCol &d, int64_t n, bool first_rows) {
  if (d.zn != n || d.phys != c.phys || (c.phys != P_I32 && c.phys != P_I64)) return false;
  FoldStats(c, n, d.zvalid, d.zmin, d.zmax, first_rows);
  return true;
}

static void UpdateStats(Engine &e, DevColumn &c, int64_t off, int64_t n, bool first_rows, bool async = false) {
  if (n <= 0) return;
  if (c.phys == P_STR || c.phys == P_F32 || c.phys == P_F64 || c.phys == P_I128 || c.phys == P_U64 ||
      c.phys == P_INTERVAL) {
    c.stats_valid = false;
    return;
  }
  long long *o3 = (long long *)((char *)e.d_small + 3072);
  int sz = PhysSize(c.phys);
  // stats over the appended range; validity offsets are bit offsets, so use a
  // validity-free pass when the column has no NULLs
  const uint64_t *v = nullptr;
  if (c.validity && (off & 63) == 0) v = c.validity + (off >> 6);
  else if (c.validity) {
    c.stats_valid = false;
    return;
  }
  {
    ProfScope ps(e, "zone_map", (double)n * sz + (v ? n / 8.0 : 0), n);
    dev::ColumnStats((const char *)c.data + off * sz, c.phys, v, n, o3, e.stream);
  }
  if (async) {
    long long *slot = nullptr;
    if (!e.stat_slots.empty()) {
      slot = e.stat_slots.back();
      e.stat_slots.pop_back();
    } else {
      HIPCHK(hipHostMalloc((void **)&slot, 3 * sizeof(long long), hipHostMallocDefault));
    }
    HIPCHK(hipMemcpyAsync(slot, o3, 3 * sizeof(long long), hipMemcpyDeviceToHost, e.stream));
    e.pending_stats.push_back({&c, slot, n, first_rows, off + n});
    return;
  }
  long long h[3];
  HIPCHK(hipMemcpyAsync(h, o3, sizeof(h), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  FoldStats(c, n, h[2], h[0], h[1], first_rows);
}

// An empty fixed-width table column takes over the pool blocks of a result
// column (values, and the bitmap when there is one) instead of allocating and
// copying: CREATE TABLE AS / INSERT ... SELECT into a new table then costs the
// query plus the zone-map pass.  A block is adopted at most once per append
// (SELECT x, x) and only when it starts at the column's pointer; string
// columns and blocks far larger than the rows still take the copy.
static bool AdoptResultColumn(DevColumn &c, const DCol &d, int64_t n, std::vector<const void *> &taken) {
  if (c.phys == P_STR || d.phys != c.phys || c.data || c.validity || c.capacity) return false;
  auto owner_of = [&](const void *p) -> DevBufPtr {
    if (!p) return nullptr;
    for (auto &o : d.owners)
      if (o && o->p == p && o->pool) return o;
    return nullptr;
  };
  DevBufPtr db = owner_of(d.data), vb = owner_of(d.validity);
  if (!db || (d.validity && !vb)) return false;
  for (const void *p : taken)
    if (p == db->p || (vb && p == vb->p)) return false;
  int64_t cap = (int64_t)(db->bytes / PhysSize(c.phys));
  if (vb) cap = std::min<int64_t>(cap, (int64_t)(vb->bytes / 8) * 64);
  // (a selective filter's output block is sized for every input row: keep at
  // most twice what the rows need, as Grow's doubling would)
  if (cap < n || db->bytes > 2 * (size_t)n * PhysSize(c.phys) + ((size_t)2 << 20)) return false;
  taken.push_back(db->p);
  c.data = db->p;
  c.data_owner = db;
  if (vb) {
    taken.push_back(vb->p);
    c.validity = (uint64_t *)vb->p;
    c.validity_owner = vb;
  }
  c.capacity = cap;
  return true;
}

static void AppendDRel(Engine &e, Table &t, const DRel &r, const std::vector<int> &col_map) {
  int64_t n = r.n, old = t.nrows;
  if (n <= 0) return;
  std::vector<const void *> taken;
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    DevColumn &c = t.cols[tc];
    int src = col_map[tc];
    if (old == 0 && src >= 0 && AdoptResultColumn(c, r.cols[src], n, taken)) {
      if (!FoldKernelStats(c, r.cols[src], n, true)) UpdateStats(e, c, 0, n, true);
      continue;
    }
    Grow(e, c, old, old + n);
    if (src < 0) {
      // column not provided: NULLs
      EnsureValidity(e, c, old);
      auto zeros = Alloc(e, Words64(n) * 8, true);
      dev::BitmapAppend(c.validity, old, (const uint64_t *)zeros->p, n, e.stream);
      if (c.phys == P_STR) {
        std::vector<int64_t> offs(n + 1, c.chars_len);
        // offsets already hold old entries; append n equal offsets
        HIPCHK(hipMemcpyAsync(c.offsets + old + 1, offs.data(), n * 8, hipMemcpyHostToDevice, e.stream));
      }
      HIPCHK(hipStreamSynchronize(e.stream));
      c.null_count += n;
      continue;
    }
    const DCol &d = r.cols[src];
    if (d.phys != c.phys) ThrowError("Internal", "append: physical type mismatch");
    if (c.phys == P_STR) {
      int64_t need = c.chars_len + d.chars_len;
      if (need > c.chars_cap) {
        int64_t cap = std::max<int64_t>(need, std::max<int64_t>(4096, c.chars_cap * 2));
        char *nc = nullptr;
        HIPCHK(hipMalloc(&nc, cap));
        if (c.chars_len) HIPCHK(hipMemcpyAsync(nc, c.chars, c.chars_len, hipMemcpyDeviceToDevice, e.stream));
        HIPCHK(hipStreamSynchronize(e.stream));
        c.chars_owner = DevOwned(e, nc);
        c.chars = nc;
        c.chars_cap = cap;
      }
      if (d.chars_len) HIPCHK(hipMemcpyAsync(c.chars + c.chars_len, d.chars, d.chars_len, hipMemcpyDeviceToDevice, e.stream));
      dev::RebaseOffsets(d.offsets + 1, c.offsets + old + 1, n, c.chars_len, e.stream);
      c.chars_len += d.chars_len;
    } else {
      int sz = PhysSize(c.phys);
      ProfScope ps(e, "append_copy", 2.0 * n * sz, n);
      HIPCHK(hipMemcpyAsync((char *)c.data + old * sz, d.data, (size_t)n * sz, hipMemcpyDeviceToDevice, e.stream));
    }
    if (d.validity) {
      EnsureValidity(e, c, old);
      dev::BitmapAppend(c.validity, old, d.validity, n, e.stream);
    } else if (c.validity) {
      dev::BitmapAppend(c.validity, old, nullptr, n, e.stream);
    }
    if (!FoldKernelStats(c, d, n, old == 0)) UpdateStats(e, c, old, n, old == 0);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  t.nrows = old + n;
  for (auto &c : t.cols) UpdateScanCodes(e, c, t.nrows);
}

void ExecuteInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map) {
  if (t.sharded()) return ShardedInsertSelect(c, t, s, col_map);
  auto t0 = std::chrono::steady_clock::now();
  Engine &e = Eng(c);
  BeginProfile(c, e);  // the statement's kernels (query, append copy, zone map) become last_profile
  DRel r;
  if (IsHostConstantSelect(s)) {
    ResultPtr hr = HostConstantSelect(s);
    r.n = hr->nrows;
    for (auto &hc : hr->cols) {
      DCol d;
      UploadHostColumn(e, hc, hr->nrows, d);
      r.cols.push_back(d);
    }
  } else {
    struct Want {
      Engine &e;
      ~Want() { e.want_zone_maps = false; }
    } want{e};
    e.want_zone_maps = true;
    MarkSetScope marks(e, c);
    r = RunSelectDev(e, c, s);
  }
  AppendCast(e, t, r, col_map);
  FinishProfile(c, e, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// r's columns (col_map[table column] = column of r, or -1) cast to the table
// types on the device where they differ, then appended
void AppendCast(Engine &e, Table &t, DRel r, const std::vector<int> &col_map) {
  // cast columns to the table types on device when they differ
  std::vector<BExprPtr> casts;
  bool need = false;
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    int src = col_map[tc];
    if (src < 0) continue;
    if (!(r.cols[src].type == t.cols[tc].type)) need = true;
  }
  if (need) {
    std::vector<BExprPtr> exprs;
    std::vector<int> map2(t.cols.size(), -1);
    for (size_t tc = 0; tc < t.cols.size(); tc++) {
      int src = col_map[tc];
      if (src < 0) continue;
      auto col = std::make_shared<BExpr>();
      col->kind = BExpr::COL;
      col->col = src;
      col->type = r.cols[src].type;
      BExprPtr x = col;
      if (!(col->type == t.cols[tc].type)) {
        auto cst = std::make_shared<BExpr>();
        cst->kind = BExpr::FUNC;
        cst->op = B_CAST;
        cst->type = t.cols[tc].type;
        cst->ch = {col};
        x = cst;
      }
      map2[tc] = (int)exprs.size();
      exprs.push_back(x);
    }
    r = FilterProject(e, r, nullptr, exprs);
    AppendDRel(e, t, r, map2);
  } else {
    AppendDRel(e, t, r, col_map);
  }
  CheckError(e);
}

// memcpy split over a few host threads (one thread tops out near 10 GB/s)
static void ParallelMemcpy(void *dst, const void *src, size_t bytes) {
  const size_t kMinPart = (size_t)2 << 20;
  int nt = (int)std::min<size_t>(8, bytes / kMinPart);
  if (nt <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  size_t part = (bytes / nt + 63) & ~(size_t)63;
  for (int i = 0; i < nt; i++) {
    size_t b = (size_t)i * part;
    if (b >= bytes) break;
    size_t len = std::min(part, bytes - b);
    th.emplace_back([=] { memcpy((char *)dst + b, (const char *)src + b, len); });
  }
  for (auto &t : th) t.join();
}

// Host -> device through the pinned ring: slot k is refilled only after its
// previous DMA (event) has completed, so copy-in and DMA overlap.
static void StageH2D(Engine &e, void *dst, const void *src, size_t bytes) {
  // Default: hand the pageable source to the runtime's own staged DMA — 14.5
  // GB/s on the C4 ingest vs 12.6 for this ring with 8 copy threads
  // (MI355X box, 1e8 INT64 rows).  MBX_INGEST=staged selects the ring.
  const char *mode = Knob("MBX_INGEST");
  if (!mode || strcmp(mode, "staged") != 0) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e.stream));
    return;
  }
  if (!e.h_stage[0]) {
    for (int i = 0; i < Engine::kStageSlots; i++) {
      HIPCHK(hipHostMalloc((void **)&e.h_stage[i], Engine::kStageBytes, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&e.stage_ev[i], hipEventDisableTiming));
      HIPCHK(hipEventRecord(e.stage_ev[i], e.stream));
    }
  }
  size_t done = 0;
  int slot = 0;
  while (done < bytes) {
    size_t b = std::min(Engine::kStageBytes, bytes - done);
    HIPCHK(hipEventSynchronize(e.stage_ev[slot]));
    ParallelMemcpy(e.h_stage[slot], (const char *)src + done, b);
    HIPCHK(hipMemcpyAsync((char *)dst + done, e.h_stage[slot], b, hipMemcpyHostToDevice, e.stream));
    HIPCHK(hipEventRecord(e.stage_ev[slot], e.stream));
    done += b;
    slot = (slot + 1) % Engine::kStageSlots;
  }
}

// Bulk appender (duckdb_mbx_append_column / _commit): every column arrives in
// its physical layout and is DMA'd straight to its place at the table's end
// (no intermediate device relation, no D2D append copy).
void AppendRawColumns(Connection &c, Table &t, const std::vector<const void *> &vals,
                      const std::vector<const uint8_t *> &valid, int64_t n, bool sync) {
  if (t.sharded()) {  // into the target part(s), split where a part fills up
    // the caller reuses the buffer of its previous flush once this returns, and
    // that flush may have gone to another shard's stream: settle every shard
    // (Eng of the target shard alone would wait only for its own stream)
    SettleAppends(c);
    int64_t off = 0;
    while (off < n) {
      const int k = TargetPart(c, t);
      int64_t m = n - off;
      if (c.opts.shard_rows > 0 && k + 1 < (int)t.parts.size())
        m = std::min<int64_t>(m, std::max<int64_t>(1, c.opts.shard_rows - t.parts[k]->nrows));
      std::vector<const void *> v2;
      std::vector<const uint8_t *> b2;
      for (size_t tc = 0; tc < t.cols.size(); tc++) {
        v2.push_back((const char *)vals[tc] + (size_t)off * PhysSize(t.cols[tc].phys));
        b2.push_back(valid[tc] ? valid[tc] + off : nullptr);
      }
      AppendRawColumns(*c.shards[k], *t.parts[k], v2, b2, m, sync);
      off += m;
      SyncRows(t);
    }
    return;
  }
  Engine &e = Eng(c);
  const int64_t old = t.nrows;
  if (n <= 0) return;
  for (size_t tc = 0; tc < t.cols.size(); tc++)
    if (t.cols[tc].phys == P_STR || t.cols[tc].phys == P_INTERVAL)
      ThrowError("Invalid Input", "append_column: only fixed-width columns are supported");
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    DevColumn &col = t.cols[tc];
    Grow(e, col, old, old + n);
    const int sz = PhysSize(col.phys);
    StageH2D(e, (char *)col.data + (size_t)old * sz, vals[tc], (size_t)n * sz);
    const uint8_t *vb = valid[tc];
    if (vb && memchr(vb, 0, (size_t)n) != nullptr) {
      std::vector<uint64_t> bm(Words64(n), 0);
      for (int64_t i = 0; i < n; i++)
        if (vb[i]) bm[i >> 6] |= 1ull << (i & 63);
      auto tmp = Alloc(e, bm.size() * 8);
      HIPCHK(hipMemcpyAsync(tmp->p, bm.data(), bm.size() * 8, hipMemcpyHostToDevice, e.stream));
      EnsureValidity(e, col, old);
      dev::BitmapAppend(col.validity, old, (const uint64_t *)tmp->p, n, e.stream);
      HIPCHK(hipStreamSynchronize(e.stream));  // bm / tmp lifetime
    } else if (col.validity) {
      dev::BitmapAppend(col.validity, old, nullptr, n, e.stream);
    }
    UpdateStats(e, col, old, n, old == 0, !sync);
  }
  t.nrows = old + n;
  if (!sync) {  // DMA + stats in flight; SettlePending waits for them and folds the stats
    e.inflight_h2d = true;
    return;
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  for (auto &col : t.cols) UpdateScanCodes(e, col, t.nrows);
  CheckError(e);
}

void SettleAppends(Connection &c) {
  if (c.engine && c.engine->has_gpu) SettlePending(*c.engine);
  for (auto &sc : c.shards) SettleAppends(*sc);
}

void *HostPinnedAlloc(size_t bytes) {
  void *p = nullptr;
  HIPCHK(hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable));  // any device of the process
  return p;
}
void HostPinnedFree(void *p) {
  if (p) (void)hipHostFree(p);
}

void AppendHostBatch(Connection &c, Table &t, const HostBatch &b) {
  if (t.sharded()) {
    const int k = TargetPart(c, t);
    AppendHostBatch(*c.shards[k], *t.parts[k], b);
    SyncRows(t);
    return;
  }
  Engine &e = Eng(c);
  DRel r;
  r.n = b.nrows;
  std::vector<int> map;
  for (size_t i = 0; i < b.cols.size(); i++) {
    DCol d;
    UploadHostColumn(e, b.cols[i], b.nrows, d);
    r.cols.push_back(d);
    map.push_back((int)i);
  }
  AppendDRel(e, t, r, map);
}
}  // namespace mbx
