function [pk,vk,ak,K_T_used,scene_status,log] = feedbackTransition(po,pf,prm,K_T_max,error_tol,trigger_p,trigger_v,reanchor,noise_p,noise_v,seed,wind,pushes)
% Event-triggered feedback (no reference counterpart): disturbedTransition under a feedback policy -- the rule include/dmpc_hip.h pins.  Every
% commanded agent plans from its own prediction while the vehicle tracks it; the planner starts from the vehicle's true state again only on an
% EVENT: the tracking error is above trigger_p (metres) in position or above trigger_v (m/s) in velocity.  trigger = 0: feed back on every column
% (disturbedTransition); Inf: never (open loop).  reanchor (default 1): an event also shifts the agent's announced plan onto the true state.
% po: 3 x N (or 1 x 3 x N); pf: 3 x N_cmd, N_cmd <= N (the vehicles behind the commanded ones are static obstacles).  prm: a dmpc_params_struct.
% noise_p, noise_v, seed, wind, pushes: the disturbance, as disturbedTransition takes it; without one the policy is inert.
% pk, vk, ak (3 x K_T_max x N_cmd), K_T_used, scene_status: as 'transition'; the histories hold the true states.
% log: a struct of the last flight's report -- event_count, event_first, event_last (1 x N_cmd; history columns, 0-based as K_T_used counts them,
% -1: none), dev_p_max, dev_v_max (the largest tracking error seen, events included) and their columns dev_p_col, dev_v_col, and xh_p, xh_v, e_p,
% e_v (3 x N_cmd): the planning state and the tracking error at the last column.
po = reshape(po,3,[]); pf = reshape(pf,3,[]);
if nargin < 8 || isempty(reanchor), reanchor = 1; end
if nargin < 9 || isempty(noise_p), noise_p = 0; end
if nargin < 10 || isempty(noise_v), noise_v = 0; end
if nargin < 11 || isempty(seed), seed = 0; end
if nargin < 12, wind = []; end
if nargin < 13, pushes = []; end
log = struct();
[pk,vk,ak,K_T_used,scene_status,log.event_count,log.event_first,log.event_last,log.dev_p_max,log.dev_p_col,log.dev_v_max,log.dev_v_col, ...
    log.xh_p,log.xh_v,log.e_p,log.e_v] = dmpc_mex('transition_feedback', prm, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, ...
    noise_p, noise_v, seed, wind, pushes);
end
