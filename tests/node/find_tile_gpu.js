"use strict";
// GPU test: findTile through the Node host.  stdin: {"labels": [str], "single": n,
// "docs": [{"initialText", "newCalc", "msgs": [[clientId, seq, refSeq, msn, type,
// contents], ...], "cuts": [int]}]}.  At each checkpoint (cuts[k] messages of every
// document applied) it asks, in ONE MergeTreeEngine.findTiles call for all
// documents, labels and both directions, every start position the golden vectors
// record (preceding [0, length] and length + 5, following [0, length)), and for
// the first `single` documents the same through BatchClient.findTile one by one.
// Prints one JSON line: per doc and checkpoint {length, text
// (getTextWithPlaceholders), q: {label: [preceding positions, following
// positions]}, hits: [[pos, properties, getId(), refType]], single: q again or
// null, sliceOk}.
const fs = require("fs");
const { MergeTreeEngine } = require("../../fluidframework_amd/node");
const { asMsg } = require("./fixtures");

const input = JSON.parse(fs.readFileSync(0, "utf8"));
const eng = new MergeTreeEngine({ nKeys: 8 });
const docs = input.docs.map((d) => ({ d, c: eng.createClient(d.initialText, { newLengthCalc: !!d.newCalc }), applied: 0, cps: [] }));
const nCp = Math.max(...input.docs.map((d) => d.cuts.length));
for (let k = 0; k < nCp; k++) {
  for (const o of docs) for (; o.applied < o.d.cuts[k]; o.applied++) o.c.applyMsg(asMsg(o.d.msgs[o.applied]));
  const queries = [], slots = [];
  docs.forEach((o, di) => {
    const length = o.c.getLength();
    const text = o.c.getTextWithPlaceholders();
    const cp = { length, text, q: {}, hits: new Map(), single: null,
      sliceOk: o.c.getTextWithPlaceholders(3, 40) === text.substring(3, 40) && o.c.getTextWithPlaceholders(5) === text.substring(5) };
    for (const label of input.labels) {
      cp.q[label] = [[], []];
      for (let p = 0; p <= length + 1; p++) {
        queries.push({ client: o.c, startPos: p <= length ? p : length + 5, tileLabel: label });  // preceding by default
        slots.push([cp, label, 0]);
      }
      for (let p = 0; p < length; p++) {
        queries.push({ client: o.c, startPos: p, tileLabel: label, preceding: false });
        slots.push([cp, label, 1]);
      }
    }
    if (di < input.single) {
      cp.single = {};
      for (const label of input.labels) {
        const pre = [], fol = [];
        for (let p = 0; p <= length + 1; p++) {
          const r = p === 0 ? o.c.findTile(undefined, label) : o.c.findTile(p <= length ? p : length + 5, label);
          pre.push(r === undefined ? -1 : r.pos);
        }
        for (let p = 0; p < length; p++) {
          const r = o.c.findTile(p, label, false);
          fol.push(r === undefined ? -1 : r.pos);
        }
        cp.single[label] = [pre, fol];
      }
    }
    o.cps.push(cp);
  });
  const res = eng.findTiles(queries);
  res.forEach((r, i) => {
    const [cp, label, dir] = slots[i];
    cp.q[label][dir].push(r === undefined ? -1 : r.pos);
    if (r !== undefined) cp.hits.set(r.pos, [r.pos, r.tile.properties === undefined ? null : r.tile.properties, r.tile.getId(), r.tile.refType]);
  });
}
const out = docs.map((o) => o.cps.map((cp) => Object.assign({}, cp, { hits: [...cp.hits.values()].sort((a, b) => a[0] - b[0]) })));
process.stdout.write(JSON.stringify({ docs: out }) + "\n");
eng.close();
