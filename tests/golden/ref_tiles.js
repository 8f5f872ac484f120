#!/usr/bin/env node
// ref_tiles.js — Client.findTile answers of the REFERENCE merge-tree itself
// (TEST INFRASTRUCTURE of tests/golden/make_tile_golden.py; runs only where the
// type-erased reference is, oracle/_ref/ts, loaded as oracle/ref_replay.js
// loads it).
//
// A document is replayed as test/client.replay.spec.ts does for its observer
// "A" (initial text inserted locally, then Client.applyMsg per message).  After
// each of the message counts in `cuts` it records the own view's length,
// getTextWithPlaceholders (MergeTreeTextHelper with placeholder " ") and, for
// every label and both directions, client.findTile(p, label, preceding)'s
// position (-1: undefined), run-length encoded over p:
//   preceding: p in [0, length], then length + 5
//   following: p in [0, length)
// plus getPropertiesAtPosition(pos) of every position that was an answer.
//
// stdin:  {"labels": [str], "docs": [{"initialText", "newCalc", "msgs": [[clientId, seq, refSeq, msn, type, contents]], "cuts": [int]}]}
// stdout: {"docs": [{"error": str|null, "cps": [{"length", "text", "q": {label: [preRle, folRle]}, "hits": [[pos, props]]}]}]}
"use strict";
const path = require("path");
const fs = require("fs");

const refdir = process.argv[2] || path.join(__dirname, "..", "..", "oracle", "_ref", "ts");
const { Client } = require(path.join(refdir, "client.js"));
const { TextSegment } = require(path.join(refdir, "textSegment.js"));
const { Marker } = require(path.join(refdir, "mergeTreeNodes.js"));
const { MergeTreeTextHelper } = require(path.join(refdir, "MergeTreeTextHelper.js"));

function specToSegment(spec) {
  const t = TextSegment.fromJSONObject(spec);
  if (t) return t;
  const m = Marker.fromJSONObject(spec);
  if (m) return m;
  throw new Error(`Unrecognized IJSONSegment type: '${JSON.stringify(spec)}'`);
}

const logger = { send() {}, sendTelemetryEvent() {}, sendErrorEvent() {}, sendPerformanceEvent() {} };

function rle(xs) {
  const out = [];
  for (const x of xs) {
    if (out.length && out[out.length - 2] === x) out[out.length - 1]++;
    else out.push(x, 1);
  }
  return out;
}

function checkpoint(client, labels) {
  const length = client.getLength();
  const helper = new MergeTreeTextHelper(client._mergeTree);
  const text = helper.getText(client.getCurrentSeq(), client.getClientId(), " ");
  const q = {};
  const hitPos = new Set();
  const ask = (p, label, preceding) => {
    const r = client.findTile(p, label, preceding);
    if (r === undefined) return -1;
    hitPos.add(r.pos);
    return r.pos;
  };
  for (const label of labels) {
    const pre = [];
    for (let p = 0; p <= length; p++) pre.push(ask(p, label, true));
    pre.push(ask(length + 5, label, true));
    const fol = [];
    for (let p = 0; p < length; p++) fol.push(ask(p, label, false));
    q[label] = [rle(pre), rle(fol)];
  }
  // a copy: getPropertiesAtPosition hands out the segment's own object, which later annotates change
  const hits = [...hitPos].sort((a, b) => a - b)
    .map((p) => [p, JSON.parse(JSON.stringify(client.getPropertiesAtPosition(p) || null))]);
  return { length, text, q, hits };
}

function replayDoc(d, labels) {
  const client = new Client(specToSegment, logger, d.newCalc ? { mergeTreeUseNewLengthCalculations: true } : undefined);
  if (d.initialText) client.insertSegmentLocal(0, new TextSegment(d.initialText));
  client.startOrUpdateCollaboration("A");
  const cps = [];
  let applied = 0;
  try {
    for (const cut of d.cuts) {
      for (; applied < cut; applied++) {
        const m = d.msgs[applied];
        client.applyMsg({ clientId: m[0], sequenceNumber: m[1], referenceSequenceNumber: m[2],
          minimumSequenceNumber: m[3], type: m[4], contents: m[5] });
      }
      cps.push(checkpoint(client, labels));
    }
  } catch (e) {
    return { error: String(e && e.message ? e.message : e), applied, cps: [] };
  }
  return { error: null, applied, cps };
}

const input = JSON.parse(fs.readFileSync(0, "utf8"));
process.stdout.write(JSON.stringify({ docs: input.docs.map((d) => replayDoc(d, input.labels)) }));
