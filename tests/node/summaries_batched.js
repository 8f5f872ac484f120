"use strict";
// MergeTreeEngine.summarizeAll (mte_read_segment_lists) on the engine: documents
// with text of several property sets, markers and remote removes on both sides
// of minSeq, replayed by one flush.  One summarizeAll per format must give,
// client by client, the blobs client.summarizeV1() / client.summarizeLegacy()
// give, with no per-document readSegments call made.
//   argv[2] documents, argv[3] messages per document.
// Prints one JSON line.
const path = require("path");
const { MergeTreeEngine } = require("../../fluidframework_amd/node");

const nDocs = Number(process.argv[2] || 50);
const nMsgs = Number(process.argv[3] || 80);
const root = path.join(__dirname, "..", "..");
const deviceAddon = require(path.join(root, "fluidframework_amd", "_lib", "mte_napi.node"));

// mulberry32 (as oracle/ref_farm.js)
function rng(seed) {
  let a = seed >>> 0;
  const next = () => {
    a = (a + 0x6d2b79f5) >>> 0;
    let t = a;
    t = Math.imul(t ^ (t >>> 15), t | 1);
    t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
  };
  return { next, int: (lo, hi) => lo + Math.floor(next() * (hi - lo + 1)) };
}

const REMOTE = ["B", "C", "D"];
const PROPS = [undefined, { bold: true }, { bold: true, size: 3 }];

// one document's stream: the window's minSeq trails by up to 12 messages, so
// the final state holds segments and tombstones on both sides of it
function stream(d) {
  const R = rng(104729 * (d + 1));
  const text = "abcdefghijklmnopqrstuvwxyz0123456789".slice(0, 24 + R.int(0, 12));
  let len = text.length, seq = 0;
  const msgs = [];
  for (let i = 0; i < nMsgs; i++) {
    seq++;
    let contents;
    const x = R.next();
    if (len < 10 || x < 0.5) {
      const props = PROPS[R.int(0, 2)];
      if (x < 0.08) {
        contents = { type: 0, pos1: R.int(0, len), seg: props ? { marker: { refType: 1 }, props } : { marker: { refType: 1 } } };
        len += 1;
      } else {
        const t = (R.next() < 0.15 ? "q\n" : "uvwxyz").slice(0, R.int(1, 6));
        contents = { type: 0, pos1: R.int(0, len), seg: props ? { text: t, props } : t };
        len += t.length;
      }
    } else if (x < 0.8) {
      const a = R.int(0, len - 1), b = Math.min(len, a + R.int(1, 5));
      contents = { type: 1, pos1: a, pos2: b };
      len -= b - a;
    } else {
      const a = R.int(0, len - 1), b = Math.min(len, a + R.int(1, 8));
      contents = { type: 2, pos1: a, pos2: b, props: { size: R.int(1, 3) } };
    }
    msgs.push({ clientId: REMOTE[R.int(0, 2)], sequenceNumber: seq, referenceSequenceNumber: seq - 1,
      minimumSequenceNumber: Math.max(0, seq - 1 - (d % 13)), type: "op", contents });
  }
  return { text, msgs };
}

const counted = Object.assign({}, deviceAddon);
const calls = { readSegments: 0, readSegmentLists: 0 };
counted.readSegments = (...a) => { calls.readSegments++; return deviceAddon.readSegments(...a); };
counted.readSegmentLists = (...a) => { calls.readSegmentLists++; return deviceAddon.readSegmentLists(...a); };
for (const k of ["findTiles", "readTexts", "propsAt", "readRefPositions"]) counted[k] = deviceAddon[k];
const e = new MergeTreeEngine({ nKeys: 4, addon: counted });
const streams = [];
for (let d = 0; d < nDocs; d++) streams.push(stream(d));
const clients = streams.map((s) => e.createClient(s.text, { newLengthCalc: true, longClientId: "A" }));
e.start();
streams.forEach((s, i) => { for (const m of s.msgs) clients[i].applyMsg(m); });
e.flush();
e.sync();

const v1 = e.summarizeAll(clients);
const legacy = e.summarizeAll(clients.slice().reverse(), { format: "legacy", chunkSize: 40 }).reverse();
const small = e.summarizeAll([clients[3], clients[3], clients[0]], { format: "v1", chunkSize: 16 });
const after = Object.assign({}, calls);

let equalV1 = 0, equalLegacy = 0, withInfo = 0, bodies = 0, first = null;
for (let d = 0; d < nDocs; d++) {
  const w1 = JSON.stringify(clients[d].summarizeV1()), g1 = JSON.stringify(v1[d]);
  const w2 = JSON.stringify(clients[d].summarizeLegacy(undefined, 40)), g2 = JSON.stringify(legacy[d]);
  if (g1 === w1) equalV1++;
  else if (!first) first = [d, "v1", g1.slice(0, 500), w1.slice(0, 500)];
  if (g2 === w2) equalLegacy++;
  else if (!first) first = [d, "legacy", g2.slice(0, 500), w2.slice(0, 500)];
  if (v1[d].header.segments.some((sp) => sp && sp.json !== undefined)) withInfo++;
  if (legacy[d].body) bodies++;
}
const smallEqual = JSON.stringify(small) === JSON.stringify([clients[3].summarizeV1(16), clients[3].summarizeV1(16),
  clients[0].summarizeV1(16)]);
let foreign = null, badFormat = null;
const other = new MergeTreeEngine({ nKeys: 4, addon: deviceAddon });
const stranger = other.createClient("x", { newLengthCalc: true });
try { e.summarizeAll([stranger]); } catch (err) { foreign = String(err.message); }
try { e.summarizeAll(clients, { format: "v2" }); } catch (err) { badFormat = String(err.message); }
process.stdout.write(JSON.stringify({ docs: nDocs, equalV1, equalLegacy, withInfo, bodies, first, smallEqual, foreign,
  badFormat, empty: e.summarizeAll([]), perDocDuringBatched: after.readSegments, batchedCalls: after.readSegmentLists,
  perDocAfter: calls.readSegments }) + "\n");
e.close();
other.close();
